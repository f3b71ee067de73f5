"""Restatement of the noise-threshold prepass (csrc/snowgpu_prepass.hip, sg_lean.h, sg_prepass_dev.h) and of the wet-ground
model (csrc/snowgpu_wet.hip) in NumPy / SciPy, in two precisions, with first-order rounding bounds and the frames that put
the kernels on their edges.

  float64      oracle.snow_oracle.estimate_laser_parameters / noise_threshold_poly / ground_water_augmentation line by line,
               keeping every intermediate (sums, means, both lines, the histogram, its row minima, the quadratic).  This is
               the reference: tests/test_prepass_reference.py holds it to the oracle's own functions bit for bit.
  longdouble   the same quantities from the same per-row float64 values (range, I / cos, cos): what the float64 answers
               round.  Bounds are measured from these.

Pure NumPy / SciPy: nothing here touches a GPU, and this module is no conftest -- the tests import it by name.  The settings the
GPU tests run (settings()) live here too, so that tests/test_prepass_reference.py can show on any machine that each of them
decides what it is listed for.

Bounds (first order, u = 2^-52; derived, not measured).  A device sum may add its n terms in any order, so
  sum of n positive terms            n u sum
  a term that holds I / cos or cos   another e_row = u (3 + max a tan a) of the term: the reference takes cos(arccos(c)), the lean
                                     chain c itself; arccos and cos are within an ulp each, which moves cos(a) by u (1 + a tan a)
                                     relatively, and I / cos carries a division on either side
  mean                               (n + 1) u mean
  centred moments, slope, intercept  (n + 3) u sum |terms|, plus the first-order effect of the two means' own bounds and of the
                                     rows' e_row; slope = sxy / sxx and intercept = ymean - slope xmean by the quotient and product rule
  quadratic                          cond(G) ((n + 4) u + e_row) max |y| at every ground range, G the normal matrix of the columns
                                     (range^2, range, 1) scaled to unit length and y = threshold cos the fitted values; plus the noise
                                     line's own bound passed through the fit (the fit is linear in the line: the fits of range cos and
                                     of cos, evaluated at the ground ranges, times the bounds of slope and intercept)
"""
from functools import lru_cache
from pathlib import Path
from types import SimpleNamespace
import re

import numpy as np

L = np.longdouble
U = 2.0 ** -52
HX, HY = 50, 2555
TILE = 1024
PLANE_W, PLANE_H = np.array([0.0, 0.0, -1.0]), -1.7
PLANE4 = [0.0, 0.0, -1.0, -1.7]
ROOT = Path(__file__).resolve().parent.parent
Q_NAMES = ("a2a2", "a2a1", "a2", "a1a1", "a1", "a2gc", "a2c", "a1gc", "a1c", "gc", "c")          # sg_lean.h: LQ_*
REC_FIELDS = ("n", "xmean", "xmean32", "ymean", "ymax", "p0", "p1") + Q_NAMES                     # k_lean_export


def small_batch_limit():
    """Largest batch for which sg_prepass_run takes k_lean_rowmin_solve (read from the source: `if (n_frames <= 16)`)."""
    src = (ROOT / "lidar_snow_sim_amd" / "csrc" / "snowgpu_prepass.hip").read_text()
    body = src[src.index('extern "C" int sg_prepass_run'):]
    m = re.search(r"if \(n_frames <= (\d+)\) \{\s*hipLaunchKernelGGL\(k_lean_rowmin_solve", body)
    assert m, "sg_prepass_run no longer switches on the frame count"
    return int(m.group(1))


# ---- frames --------------------------------------------------------------------------------------------------------
def _row_with_norm(target, dtype):
    """(x, y, z) of `dtype`, z near -1.7, whose norm, as np.linalg.norm(axis=1) computes it in that dtype, is exactly `target`."""
    dtype = np.dtype(dtype)
    t = dtype.type(target)
    assert float(t) == float(target), "target is no value of the dtype"
    steps = np.arange(-300, 301)
    for zz in (-1.7, -1.6875, -1.71875, -1.65625):
        for yy in (0.0, 0.5, 1.25, 2.0, 3.5, 5.0):
            zz, yy = dtype.type(zz), dtype.type(yy)
            x = dtype.type(np.sqrt(float(t) ** 2 - float(zz) ** 2 - float(yy) ** 2))
            cand = (x + steps * np.spacing(x)).astype(dtype)           # x and its neighbours, 300 ulps either way
            rows = np.column_stack((cand, np.full_like(cand, yy), np.full_like(cand, zz)))
            hit = np.nonzero(np.linalg.norm(rows, axis=1) == t)[0]
            if hit.size:
                return rows[hit[0]]
    raise AssertionError(f"no {dtype} row with norm {target!r}")


def x_edges():
    return np.linspace(10.0, 70.0, HX + 1)


def edge_targets(dtype):
    """Ranges on and beside the histogram's x edges: every edge k * 1.2 + 10 itself where the dtype holds it, and its two
    neighbours in the dtype (float32: the two float32 values that bracket an edge float32 cannot hold); 10 and 70 with the values
    just outside."""
    dtype = np.dtype(dtype)
    out = []
    for e in x_edges():
        t = dtype.type(e)
        if float(t) == e:
            out += [np.nextafter(t, dtype.type(-np.inf)), t, np.nextafter(t, dtype.type(np.inf))]
        else:
            below = t if float(t) < e else np.nextafter(t, dtype.type(-np.inf))
            out += [below, np.nextafter(below, dtype.type(np.inf))]
    return np.array(out, dtype)


def _level(rng, r, levels, jitter):
    base = 200.0 + 3.0 * r
    return base * rng.choice(np.asarray(levels), r.shape[0]) * (1.0 + rng.uniform(-jitter, jitter, r.shape[0]))


def road(n_ground, n_other, seed, dtype, bands=((8.0, 75.0),), dark=0.15, levels=(0.3, 0.6, 1.0, 1.5), jitter=0.02, z_half=0.49,
         blank_tile=None, edge_rows=False, single_bin=(), sort_channels=False):
    """N x 5 rows (x, y, z, intensity, channel) over the plane ([0, 0, -1], -1.7), N = n_ground + n_other (+ the edge rows).

    Ground rows: range drawn from `bands`, z = -1.7 +- z_half, I / cos from a few levels per range (200 + 3 range, times a level, times
    1 +- jitter), a share `dark` of them with I / cos in [0.5, 4.5] (below the histogram).  Other rows: z in [0.5, 3].  All shuffled
    together (sort_channels: then stably sorted by channel), channels 0 .. 63, ranges below 119 m.
    blank_tile: no ground row among rows [1024 t, 1024 t + 1024).  edge_rows: a ground row on and beside every x edge (edge_targets).
    single_bin: (range row, count) -- `count` ground rows in that histogram row with ONE I / cos, and no other ground row in it."""
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(seed)
    lo = np.array([b[0] for b in bands]); hi = np.array([b[1] for b in bands])
    pick = rng.choice(len(bands), n_ground, p=(hi - lo) / (hi - lo).sum())
    r = rng.uniform(lo[pick], hi[pick])
    xe = x_edges()
    for row, _ in single_bin:                                           # keep the generic rows out of the single-bin histogram rows
        inside = (r >= xe[row]) & (r < xe[row + 1])
        r[inside] += 1.2 if row + 1 < HX - 1 else -1.2
    z = -1.7 + rng.uniform(-z_half, z_half, n_ground)
    norm = _level(rng, r, levels, jitter)
    is_dark = rng.uniform(size=n_ground) < dark
    norm[is_dark] = rng.uniform(0.5, 4.5, int(is_dark.sum()))
    az = rng.uniform(-np.pi, np.pi, n_ground)
    rho = np.sqrt(r * r - z * z)
    ground = np.column_stack((rho * np.cos(az), rho * np.sin(az), z, norm * (-z / r)))
    extra = []
    if edge_rows:
        for t in edge_targets(dtype):
            xyz = _row_with_norm(t, dtype).astype(np.float64)
            nv = float(_level(rng, np.array([float(t)]), levels, jitter)[0])
            extra.append([xyz[0], xyz[1], xyz[2], nv * (-xyz[2] / float(t))])
    for row, count in single_bin:
        rr = rng.uniform(xe[row] + 0.1, xe[row + 1] - 0.1, count)
        zz = np.full(count, -1.7)
        a = rng.uniform(-np.pi, np.pi, count)
        rh = np.sqrt(rr * rr - zz * zz)
        nv = (200.0 + 3.0 * xe[row]) * 0.8
        for i in range(count):
            extra.append([rh[i] * np.cos(a[i]), rh[i] * np.sin(a[i]), zz[i], nv * (1.7 / rr[i])])
    if extra:
        ground = np.vstack((ground, np.array(extra)))
    # the frame's largest I / cos belongs to a row inside the histogram's ranges: the last y edge is then hit, on both sides, by construction
    rg = np.sqrt((ground[:, :3] ** 2).sum(axis=1))
    inside = np.nonzero((rg[:n_ground] > 10.5) & (rg[:n_ground] < 69.5))[0]
    if inside.size:
        cosv = -ground[:, 2] / rg
        top = inside[np.argmax((ground[:, 3] / cosv)[inside])]
        ground[top, 3] = 1.01 * np.max(ground[:, 3] / cosv) * cosv[top]
    ng = ground.shape[0]
    ro = rng.uniform(3.0, 100.0, n_other)
    zo = rng.uniform(0.5, 3.0, n_other)
    ao = rng.uniform(-np.pi, np.pi, n_other)
    rh = np.sqrt(ro * ro - zo * zo)
    other = np.column_stack((rh * np.cos(ao), rh * np.sin(ao), zo, rng.uniform(1.0, 250.0, n_other)))
    n = ng + n_other
    slots = np.arange(n)
    if blank_tile is not None:
        slots = slots[(slots < blank_tile * TILE) | (slots >= (blank_tile + 1) * TILE)]
        assert slots.size >= ng
    tiles = [t for t in range((n + TILE - 1) // TILE) if t != blank_tile]
    first = np.array([rng.choice(slots[slots // TILE == t]) for t in tiles[::-1][:ng]], dtype=np.int64)   # a ground row in every tile it may have one (the last tile first)
    gpos = np.concatenate((first, rng.permutation(np.setdiff1d(slots, first))[:ng - len(first)]))
    is_g = np.zeros(n, bool); is_g[gpos] = True
    rows = np.empty((n, 5))
    rows[is_g, :4] = ground[rng.permutation(ng)]
    rows[~is_g, :4] = other
    rows[:, 4] = rng.integers(0, 64, n)
    if sort_channels:
        rows = rows[np.argsort(rows[:, 4], kind="stable")]
    out = rows.astype(dtype)
    if edge_rows:                                                       # the cast keeps the edge rows' coordinates: they are values of the dtype
        assert np.isin(edge_targets(dtype), np.linalg.norm(out[:, :3], axis=1)).all()
    return out


# ---- the estimate --------------------------------------------------------------------------------------------------
def ground_rows(pc, w=PLANE_W, h=PLANE_H, delta=0.5, flat_earth=False, promote=False):
    """simulation.py:450-455 (promote=False: the snowfall prepass, rows keep their dtype) / augmentation.py:46-63 (promote=True: the wet
    model, whose np.hstack with the float64 height column makes the ground rows float64): ground mask, the ground rows, range, incident
    angle, I / cos(angle), cos(angle) -- the reference's statements."""
    w = np.asarray(w, np.float64)
    hog = np.matmul(pc[:, :3], w)
    ground = np.logical_and(hog + h < delta, hog + h > -delta)
    g = pc[ground]
    if promote:
        g = g.astype(np.float64)
    if not flat_earth:
        angle = np.arccos(np.divide(np.matmul(g[:, :3], w), np.linalg.norm(g[:, :3], axis=1) * np.linalg.norm(w)))
    else:
        angle = np.arccos(-np.divide(np.matmul(g[:, :3], np.asarray([0, 0, 1])), np.linalg.norm(g[:, :3], axis=1) * np.linalg.norm([0, 0, 1])))
    dist = np.linalg.norm(g[:, :3], axis=1)
    return SimpleNamespace(mask=ground, rows=g, hog=hog + h, dist=dist, angle=angle, norm=g[:, 3] / np.cos(angle), cos=np.cos(angle))


def histogram(dist, norm):
    """augmentation.py:232-241: histogram with its empty bins set to the ground count, edges, first minimum per range row, the usable rows."""
    hist, xedges, yedges = np.histogram2d(dist, norm, bins=(HX, HY), range=((10, 70), (5, np.abs(np.max(norm)))))
    raw = hist.copy()
    hist[np.where(hist == 0)] = len(dist)
    ymins = np.argmin(hist, axis=1)
    min_vals = yedges[ymins]
    idx = np.where(min_vals > 5)
    x = (xedges[idx] + xedges[idx[0] + 1]) / 2
    tied = np.array([(hist[r] == hist[r, ymins[r]]).sum() for r in range(HX)])
    return SimpleNamespace(hist=hist, raw=raw, xedges=xedges, yedges=yedges, ymins=ymins, min_vals=min_vals, usable=idx[0], x=x, y=min_vals[idx], tied=tied)


def _scaled_lstsq(cols, y):
    """np.polyfit's solve on given columns: scale them to unit length, lstsq, divide by the scale."""
    lhs = np.column_stack(cols).astype(np.float64)
    scale = np.sqrt((lhs * lhs).sum(axis=0))
    c = np.linalg.lstsq(lhs / scale, y, rcond=len(y) * np.finfo(np.float64).eps)[0]
    return c / scale


def _columns(dist):
    """The fit's columns as the device takes them: range, and range^2 as a product in the rows' dtype (np.polyfit keeps it for the Vandermonde)."""
    return (dist * dist).astype(np.float64), dist.astype(np.float64), np.ones(len(dist))


def estimate64(g, noise_floor=0.7, power_factor=15):
    """estimate_laser_parameters + noise_threshold_poly's fit on the ground values `g` (ground_rows), in float64 NumPy / SciPy."""
    from scipy.stats import linregress
    reg = linregress(g.dist, g.norm)
    p = (np.float64(reg[0]), np.float64(reg[1]))                       # (NumPy scalars: a Python float would keep float32 ranges float32)
    h = histogram(g.dist, g.norm)
    if len(h.y) > 3:
        r2 = linregress(h.x, h.y)
        pmin = (np.float64(r2[0]), np.float64(r2[1]))
    else:
        pmin = p
    thr = noise_floor * (pmin[0] * g.dist + pmin[1])
    a2, a1, a0 = _columns(g.dist)
    y = thr * g.cos
    poly = _scaled_lstsq((a2, a1, a0), y)
    d64, c = g.dist.astype(np.float64), g.cos
    q = np.array([np.sum(a2 * a2), np.sum(a2 * a1), np.sum(a2), np.sum(a1 * a1), np.sum(a1), np.sum(a2 * (d64 * c)), np.sum(a2 * c),
                  np.sum(a1 * (d64 * c)), np.sum(a1 * c), np.sum(d64 * c), np.sum(c)])
    rec = np.concatenate(([len(g.dist), np.mean(d64), float(np.mean(g.dist)), np.mean(g.norm), np.abs(np.max(g.norm)), p[0], p[1]], q))
    return SimpleNamespace(p=p, pmin=pmin, m=len(h.y), hist=h, thr=thr, poly=poly, rec=rec, fallback=len(h.y) <= 3)


def _line_ld(x, y, dy, xm_used=None):
    """linregress's slope and intercept of (x, y) in longdouble with their first-order bounds; dy: what each y may be off by already.
    xm_used: the mean the intercept takes when it is not the mean of x (NumPy's float32 mean of a float32 column), taken as exact."""
    n = len(x)
    x, y = x.astype(L), y.astype(L)
    xm, ym = x.sum() / n, y.sum() / n
    dx, dyc = x - xm, y - ym
    sxx, sxy = (dx * dx).sum(), (dx * dyc).sum()
    slope = sxy / sxx
    b_xm = (n + 1) * U * abs(xm)
    b_ym = (n + 1) * U * np.abs(y).sum() / n + np.sum(dy) / n
    b_sxx = (n + 3) * U * sxx + 2 * b_xm * np.abs(dx).sum()
    b_sxy = (n + 3) * U * np.abs(dx * dyc).sum() + b_xm * np.abs(dyc).sum() + b_ym * np.abs(dx).sum() + (np.abs(dx) * dy).sum()
    b_slope = b_sxy / sxx + abs(sxy) * b_sxx / (sxx * sxx) + 3 * U * abs(slope)
    xu, b_xu = (xm, b_xm) if xm_used is None else (L(xm_used), 0.0)
    icpt = ym - slope * xu
    b_icpt = b_ym + abs(xu) * b_slope + abs(slope) * b_xu + 2 * U * (abs(ym) + abs(slope * xu))
    return SimpleNamespace(slope=slope, icpt=icpt, b_slope=L(b_slope), b_icpt=L(b_icpt), xm=xm, ym=ym, b_xm=L(b_xm), b_ym=L(b_ym), sxx=sxx, sxy=sxy)


def _solve3_ld(cols, y):
    """Least squares over three columns through the normal equations in longdouble (columns scaled to unit length)."""
    a = np.column_stack([c.astype(L) for c in cols])
    s = np.sqrt((a * a).sum(axis=0))
    a = a / s
    g = np.column_stack((a.T @ a, a.T @ y.astype(L)))
    for i in range(3):
        piv = i + int(np.argmax(np.abs(g[i:, i])))
        g[[i, piv]] = g[[piv, i]]
        for r in range(i + 1, 3):
            g[r] -= (g[r, i] / g[i, i]) * g[i]
    x = np.zeros(3, L)
    for i in (2, 1, 0):
        x[i] = (g[i, 3] - (g[i, i + 1:3] * x[i + 1:]).sum()) / g[i, i]
    return x / s


def estimate_ld(g, e64, noise_floor=0.7, f32_mean=False):
    """The quantities of estimate64 in np.longdouble from the same per-row float64 values, and the bound of each (module docstring).
    The discrete part (the histogram and its row minima) is taken from e64.  f32_mean: the intercept of the regression line takes
    NumPy's float32 mean of the float32 range column (the snowfall prepass on float32 rows), which the device reproduces bit for bit."""
    assert np.finfo(L).nmant > 60, "np.longdouble is no wider than float64 here: no high-precision reference"
    n = len(g.dist)
    a = g.angle.astype(L)
    e_row = U * (3.0 + float(np.max(a * np.tan(a))))
    d, y, c = g.dist.astype(L), g.norm.astype(L), g.cos.astype(L)
    xm32 = float(np.mean(g.dist)) if f32_mean else None
    ln = _line_ld(g.dist, g.norm, e_row * np.abs(y), xm_used=xm32)
    a2, a1, a0 = (v.astype(L) for v in _columns(g.dist))
    terms = (a2 * a2, a2 * a1, a2, a1 * a1, a1, a2 * (d * c), a2 * c, a1 * (d * c), a1 * c, d * c, c)
    q = np.array([t.sum() for t in terms])
    b_q = np.array([((n + 4) * U + (e_row if k >= 5 else 0.0)) * q[k] for k in range(11)])
    ymax = np.abs(np.max(y))
    rec = np.concatenate(([L(n), ln.xm, L(xm32 if f32_mean else np.mean(g.dist.astype(np.float64))), ln.ym, ymax, ln.slope, ln.icpt], q))
    b_rec = np.concatenate(([L(0), ln.b_xm, L(0) if f32_mean else ln.b_xm, ln.b_ym, e_row * ymax, ln.b_slope, ln.b_icpt], b_q))
    h = e64.hist
    if len(h.y) > 3:                                                    # the edges carry the maximum's e_row and three roundings
        mn = _line_ld(h.x, h.y, (e_row + 3 * U) * np.abs(h.y.astype(L)))
    else:
        mn = ln
    pmin, b_pmin = (mn.slope, mn.icpt), (mn.b_slope, mn.b_icpt)
    yfit = noise_floor * (pmin[0] * d + pmin[1]) * c
    poly = _solve3_ld((a2, a1, a0), yfit)
    am = np.column_stack((a2, a1, a0)).astype(np.float64)
    am = am / np.sqrt((am * am).sum(axis=0))
    cond = float(np.linalg.cond(am.T @ am))
    f_dc, f_c = _solve3_ld((a2, a1, a0), d * c), _solve3_ld((a2, a1, a0), c)
    ev = lambda co: co[0] * a2 + co[1] * a1 + co[2]                     # noqa: E731  (at the ground ranges, with the columns the fit used)
    b_poly = cond * ((n + 4) * U + e_row) * np.max(np.abs(yfit)) + noise_floor * (b_pmin[0] * np.abs(ev(f_dc)) + b_pmin[1] * np.abs(ev(f_c)))
    return SimpleNamespace(rec=rec, b_rec=b_rec, p=(ln.slope, ln.icpt), b_p=(ln.b_slope, ln.b_icpt), pmin=pmin, b_pmin=b_pmin, poly=poly,
                           poly_at=ev(poly), b_poly_at=b_poly, cond=cond, e_row=e_row, a2=a2, a1=a1)


def poly_at(poly, ld):
    """A polynomial (highest power first) at the frame's ground ranges, with the columns the fit used, in longdouble."""
    p = np.asarray(poly).astype(L)
    return p[0] * ld.a2 + p[1] * ld.a1 + p[2]


def snow_frame(pc):
    """The snowfall prepass of one frame, restated: the reference sorts by channel first (simulation.py:447), which fixes the order of
    NumPy's sums.  -> (ground values, float64 estimate, longdouble estimate)."""
    srt = pc[np.argsort(pc[:, 4], kind="stable")]
    g = ground_rows(srt)
    e = estimate64(g)
    return g, e, estimate_ld(g, e, f32_mean=pc.dtype == np.float32)


def stats_frame(pc):
    """As snow_frame for Context.prepass_stats, which takes the rows in the order they come."""
    g = ground_rows(pc)
    e = estimate64(g)
    return g, e, estimate_ld(g, e, f32_mean=pc.dtype == np.float32)


# ---- wet ground ----------------------------------------------------------------------------------------------------
def _fresnel(ain, n_in, n_out):
    a = np.clip(np.sin(ain) * n_in / n_out, -1, 1)
    aout = np.arcsin(a)
    frac = np.cos(ain) * n_in / n_out / np.cos(aout)
    rs = (n_in * np.cos(ain) - n_out * np.cos(aout)) / (n_in * np.cos(ain) + n_out * np.cos(aout))
    ts = 2 * n_in * np.cos(ain) / (n_in * np.cos(ain) + n_out * np.cos(aout))
    rp = (n_out * np.cos(ain) - n_in * np.cos(aout)) / (n_out * np.cos(ain) + n_in * np.cos(aout))
    tp = 2 * n_in * np.cos(ain) / (n_out * np.cos(ain) + n_in * np.cos(aout))
    return rs ** 2, ts ** 2 / frac, rp ** 2, tp ** 2 / frac, aout


def wet_chain(inten, angle, dist, lines, water_height, pavement_depth, noise_floor, power_factor, T=np.float64):
    """augmentation.py:90-131 per ground row from its intensity, angle, range and the two lines (p0, p1, pmin0, pmin1), in precision T
    (np.float64: the reference's statements; np.longdouble: what they round)."""
    inten, angle, dist = inten.astype(T), angle.astype(T), dist.astype(T)
    p0, p1, m0, m1 = (T(v) for v in lines)
    nair, nw = T(1.0003), T(1.33)
    rel = T(power_factor) * (p0 * dist + p1)
    thr = T(noise_floor) * (m0 * dist + m1)
    refl = inten / np.cos(angle) / rel
    rho = np.clip(refl, T(0.05), T(1))
    ras, tas, rap, tap, aaout = _fresnel(angle, nair, nw)
    rws, tws, rwp, twp, _ = _fresnel(aaout, nw, nair)
    ts = tas * rho * tws / (1 - rho * rws)
    tp = tap * rho * twp / (1 - rho * rwp)
    t = np.maximum(tp, ts)
    f = np.clip(T(water_height) / T(pavement_depth), 0, 1)
    tw = (1 - f) * refl + f * t / angle
    raw = rel * np.cos(angle) * tw
    new_i = np.clip(raw, 0, inten)
    lim = thr * np.cos(angle)
    new_i[new_i < lim] = 0
    keep = new_i > lim
    return SimpleNamespace(rel=rel, thr=thr, refl=refl, rho=rho, raw=raw, new_i=new_i, lim=lim, keep=keep, cancel=(p0 * dist, p1))


def wet_restated(pc, water_height=0.001, pavement_depth=0.0012, noise_floor=0.7, power_factor=15, flat_earth=False, delta=0.5,
                 replace=True, lines=None):
    """ground_water_augmentation (augmentation.py:25-161, 'linear') on the plane ([0, 0, -1], -1.7), with the caller's two lines instead
    of the fitted ones when `lines` is given.  -> namespace(out, src, flag, g, e64 or None, chain, chain_ld)."""
    n = pc.shape[0]
    g = ground_rows(pc, delta=delta, flat_earth=flat_earth, promote=True)
    gidx = np.where(g.mask)[0]
    if len(gidx) < 1000:
        return SimpleNamespace(out=pc.astype(np.float64), src=np.arange(n), flag=1, g=g, e64=None, chain=None, chain_ld=None, lines=None)
    e = None
    if lines is None:
        e = estimate64(g, noise_floor, power_factor)
        lines = (e.p[0], e.p[1], e.pmin[0], e.pmin[1])
    args = (g.rows[:, 3], g.angle, g.dist, lines, water_height, pavement_depth, noise_floor, power_factor)
    ch, ch_ld = wet_chain(*args), wet_chain(*args, T=L)
    keep = np.where(ch.keep)
    n_ng = n - len(gidx)
    out = np.zeros((n_ng + keep[0].shape[0], pc.shape[1]))
    out[:n_ng, :] = pc[np.logical_not(g.mask), :]
    out[n_ng:, :] = g.rows[keep]
    out[n_ng:, 3] = ch.new_i[keep]
    if replace:
        out[:, 4] = 0
    out[n_ng:, 4] = 1
    src = np.concatenate((np.where(np.logical_not(g.mask))[0], gidx[keep]))
    return SimpleNamespace(out=out, src=src, flag=0, g=g, e64=e, chain=ch, chain_ld=ch_ld, lines=lines)


# ---- settings ------------------------------------------------------------------------------------------------------
MEAN32_COUNTS = (3, 7, 8, 9, 127, 128, 129, 136, 255, 256, 257, 1000, 4099)
TILE_ROWS = (1023, 1024, 1025, 2049, 65 * TILE + 1)
M3_BANDS = ((19.7, 20.7), (40.1, 41.1), (60.5, 61.5), (8.0, 9.9), (70.5, 75.0))         # three usable range rows; the rest outside [10, 70]
M4_BANDS = M3_BANDS[:3] + ((30.5, 31.5),) + M3_BANDS[3:]
# Setting 5, fallback frames by ground count: across NumPy's 128-term leaf (129), a split at no multiple of 8 (136), three leaves (257), several
# levels of splits (1000).  Rows shuffled; the seeds are chosen so that the float32 mean of the ground ranges differs between the order the
# rows come in and the channel-sorted order the reference sums in (tests/test_prepass_reference.py asserts it).
FALLBACK_COUNTS = {129: 514, 136: 518, 257: 500, 1000: 510}            # ground rows: seed
WET_PARAMS = (
    dict(water_height=0.0, pavement_depth=0.001, flat_earth=False, replace=True, delta=0.5, noise_floor=0.7, power_factor=15),
    dict(water_height=0.0004, pavement_depth=0.001, flat_earth=True, replace=False, delta=0.5, noise_floor=0.7, power_factor=15),
    dict(water_height=0.0008, pavement_depth=0.001, flat_earth=False, replace=False, delta=0.2, noise_floor=0.7, power_factor=15),
    dict(water_height=0.001, pavement_depth=0.001, flat_earth=True, replace=True, delta=0.2, noise_floor=0.7, power_factor=15),
    dict(water_height=0.002, pavement_depth=0.001, flat_earth=False, replace=True, delta=0.5, noise_floor=0.7, power_factor=15),
    dict(water_height=0.0008, pavement_depth=0.001, flat_earth=False, replace=True, delta=0.5, noise_floor=0.5, power_factor=1.0),
    dict(water_height=0.002, pavement_depth=0.001, flat_earth=True, replace=False, delta=0.5, noise_floor=0.5, power_factor=1.0),
)
LINES = (1.0, -12.0, 2.0, -30.0)       # setting 10: both lines cross zero inside the ground ranges
LINES_PARAMS = dict(water_height=0.0008, pavement_depth=0.001, flat_earth=False, replace=True, delta=0.5, noise_floor=0.7, power_factor=15)


def _dt(tag):
    return np.float32 if tag == "f32" else np.float64


@lru_cache(maxsize=None)
def frame(name, tag):
    """The frames of the settings table by name; tag 'f32' / 'f64'."""
    dt = _dt(tag)
    s = 1 if tag == "f32" else 2
    if name.startswith("tiles"):                                        # setting 1
        n = int(name[5:])
        ng = max(3, min(n // 3, 20000))
        return road(ng, n - ng, 100 + n % 97 + s, dt, blank_tile=3 if n > 4 * TILE else None)
    if name.startswith("mean"):                                         # setting 2: ground count exact, scattered over two tiles
        k = int(name[4:])
        return road(k, 1100 if k < 900 else 600, 200 + k + s, dt, dark=0.0 if k < 10 else 0.15)
    if name == "edges":                                                 # setting 3
        return road(3000, 1500, 300 + s, dt, edge_rows=True)
    if name == "ties":                                                  # setting 4
        return road(2500, 900, 310 + s, dt, single_bin=((7, 5), (30, 1), (49, 3)))
    if name == "m3":                                                    # setting 5
        return road(1400, 800, 320 + s, dt, bands=M3_BANDS)
    if name == "m4":
        return road(1400, 800, 330 + s, dt, bands=M4_BANDS)
    if name.startswith("fb"):                                           # three usable range rows at most: the noise line falls back
        k = int(name[2:])
        return road(k, 1100 if k < 900 else 600, FALLBACK_COUNTS[k] + s, dt, bands=M3_BANDS)
    if name == "plain":
        return road(1800, 700, 340 + s, dt)
    if name == "sorted":                                                # setting 7: channel-major beside the shuffled frames
        return road(1800, 700, 350 + s, dt, sort_channels=True)
    if name == "m3sorted":
        return road(1400, 800, 360 + s, dt, bands=M3_BANDS, sort_channels=True)
    if name == "wet":                                                   # setting 8
        return road(4200, 1900, 400 + s, dt)
    if name == "wet_tiles":                                             # 65 tiles + 1: the second trip of k_wet_scan / k_pre_means / frame_sums
        return road(20000, 65 * TILE + 1 - 20000, 410 + s, dt, blank_tile=3)
    if name == "g999":                                                  # setting 9
        return road(999, 1300, 420 + s, dt)
    if name == "g1000":
        return road(1000, 1300, 430 + s, dt)
    if name == "empty":
        return np.zeros((0, 5), dt)
    if name == "lines":                                                 # setting 10
        return road(3000, 1100, 440 + s, dt, dark=0.3)
    raise KeyError(name)


FALLBACK_FRAMES = tuple(f"fb{k}" for k in FALLBACK_COUNTS)
BATCH_FRAMES = ("plain", "m3", "ties", "sorted", "m4", "tiles1025", "m3sorted", "edges", "fb136", "fb1000")


def batch_names(n):
    """Setting 6: the same frames in a batch of n (ragged: the frames differ in size)."""
    return [BATCH_FRAMES[i % len(BATCH_FRAMES)] for i in range(n)]


def concat(frames):
    off = np.concatenate(([0], np.cumsum([f.shape[0] for f in frames]))).astype(np.int64)
    return np.concatenate(frames), off
