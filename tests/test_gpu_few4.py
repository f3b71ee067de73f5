"""-m gpu: k_power_few<T, 4> (csrc/snowgpu_kernels.hip, csrc/sg_few.h with N = 4) -- the register kernel that takes the BACK run of every
region of the dict queue, i.e. the beams of the pass over all rows that met three or four flakes -- against the oracle, byte for byte:
rows, source indices, counts, stats and the status words (class populations [2 .. 5], the row kernels' redo counter [6]).

One batch of two frames (838 rows, far below 2 x 64 x 128) whose beams are CONSTRUCTED with the builders of tests/row_tier_inputs.py
(comb, umbrella, hidden) -- a region is a (frame, channel) segment, and a channel's beams stand 0.04 rad apart, each over its own flakes:
  * back runs of 0, 1, 63, 64, 65 and 129 slots (frame 0, BACK_RUNS): nothing to do, one lane, one lane short of an item, a full item,
    one slot into a second item, one slot into a third; every such channel also queues a front run of one- and two-flake beams;
  * three- and four-flake beams in turn, so every wave mixes them: comb(3), comb(4), umbrella(2), umbrella(3) -- four flakes, the nearest
    owning seven slots --, hidden(3) -- four flakes, three scatterers -- and comb(3) with one table row twice -- four flakes, the copy
    later in scan order owns nothing;
  * wedges across azimuth 0 (SEAM): comb(4), umbrella(3) and comb(3) whose wedge straddles the 0 / 2 pi seam, one flake's interval wrapping,
    the flakes before it wholly right of azimuth 0 (they keep their angles near 2 pi: the reference's dict gives the target the gap);
  * frame 1 holds back runs of 65, 1 and 0 on the same channels with other tables: the items carry their frame.
The host analysis of tests/test_row_tier_inputs.py (beam_intervals: what get_occlusions hands the dict, held to the oracle there) counts the
flakes every beam meets; from it the test derives, asserts and PRINTS the back run of every region -- a failure shows which kernel ran.

Not here: a scatterer with eight or nine slots.  With at most four flakes that takes nine or ten distinct interval ends, so an interval
that strictly contains a limit ray -- and get_occlusions clips every interval that crosses a ray to it (geometry.py:14-29): no table of
flakes gives k_power_few<T, 4> such a list.  Those lists, and the pairwise sums they need, are held bit for bit to the general path on
the host (tests/test_few4_math.py, where the functions take any list); here umbrella(3) reaches the seven slots a table can give."""
from functools import lru_cache

import numpy as np
import pytest
import torch  # noqa: F401  -- before libsnowgpu.so is loaded: PyTorch bundles its own HIP runtime, and the process must end up with one

import row_tier_inputs as rti
import test_gpu_row_tiers as trt
import test_row_tier_inputs as tri

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
W = 3e-3                                                              # wedge width at rti.BD
FRONT_MAX = 2                                                         # beams with up to two flakes take k_power_few<T, 2> (SNOWGPU_FEW)
BACK_RUNS = {3: 0, 10: 1, 17: 63, 24: 64, 31: 65, 38: 129}            # frame 0: channel -> slots of its back run
BACK_RUNS_1 = {3: 65, 10: 1, 17: 0}                                   # frame 1
FRONT_RUN = 11                                                        # one- and two-flake beams on each of these channels
SEAM = {52: ("comb", 4, 0), 53: ("umbrella", 3, 1), 54: ("comb", 3, 1)}   # channel -> kind, m, the flake whose centre lies 1e-5 rad left of azimuth 0


def _twin3(w):
    return rti.comb(3, w)                                             # (table row 2 is filed twice below)


BACK_KINDS = [("comb3", lambda w: rti.comb(3, w), 3), ("comb4", lambda w: rti.comb(4, w), 4), ("umbrella2", lambda w: rti.umbrella(2, w), 3),
              ("umbrella3", lambda w: rti.umbrella(3, w), 4), ("hidden3", lambda w: rti.hidden(3, w), 4), ("twin3", _twin3, 4)]
FRONT_KINDS = [("comb1", lambda w: rti.comb(1, w), 1), ("comb2", lambda w: rti.comb(2, w), 2), ("umbrella1", lambda w: rti.umbrella(1, w), 2)]


def _frame(runs, seam, seed, dtype, scale):
    """rows (channel-major), tables, per row the flakes it was built to meet; scale: the beams' range as a fraction of rti.D_TARGET"""
    rng = np.random.default_rng(seed)
    fix = rti.fixture_tables()
    tables = [fix[c % 4] for c in range(rti.N_LASERS)]
    az_all, d_all, ch_all, want_all = [], [], [], []
    for ch, n_back in runs.items():
        kinds = [BACK_KINDS[(i + ch) % len(BACK_KINDS)] for i in range(n_back)] + [FRONT_KINDS[i % len(FRONT_KINDS)] for i in range(FRONT_RUN)]
        order = rng.permutation(len(kinds))                           # front and back beams in any order along the channel
        flakes = []
        for slot, k in enumerate(order):
            name, make, n_meet = kinds[k]
            az = 0.3 + 0.04 * slot
            fl = rti._flakes(az, *make(W))
            if name == "twin3":
                fl = np.concatenate((fl, fl[2:3]))                    # table row 2 again, byte for byte
            flakes.append(fl)
            az_all.append(az); d_all.append(rti.D_TARGET * scale); ch_all.append(ch); want_all.append(n_meet)
        tables[ch] = np.ascontiguousarray(np.concatenate(flakes))
    for ch, (kind, m, j) in seam.items():
        c, h, rho = (rti.umbrella if kind == "umbrella" else rti.comb)(m, W)
        az = 1e-5 - c[j]
        tables[ch] = np.ascontiguousarray(rti._flakes(az, c, h, rho))
        az_all.append(az); d_all.append(rti.D_TARGET * scale); ch_all.append(ch); want_all.append(m + (kind == "umbrella"))
    free = [c for c in range(rti.N_LASERS) if c not in runs and c not in seam]
    az, d, ch = rti._ordinary(rng, free, 3, 3.0, 119.0)
    az = np.concatenate((az_all, az)); d = np.concatenate((d_all, d)); ch = np.concatenate((ch_all, ch))
    want = np.concatenate((want_all, np.full(3 * len(free), -1)))      # -1: an ordinary beam, whatever it meets
    o = np.argsort(ch, kind="stable")
    rows = rti._rows(az[o], d[o], ch[o], rng, dtype)
    return rows, tables, want[o]


@lru_cache(maxsize=None)
def _batch(dtype_name, scale=1.0):
    """the two frames, the oracle's result for each, and the host analysis: flakes met and most slots of one owner per row"""
    from oracle import snow_oracle as so
    so.build()
    dtype = np.dtype(dtype_name).type
    frames = [_frame(BACK_RUNS, SEAM, 8301, dtype, scale), _frame(BACK_RUNS_1, {}, 8302, dtype, scale)]
    refs, n_hit_all, most_all = [], [], []
    for rows, tables, want in frames:
        d, ang = tri.beam_angles_of(rows, rti.BD)
        n_hit, most = np.zeros(rows.shape[0], np.int64), np.zeros(rows.shape[0], np.int64)
        for ch in np.unique(rows[:, 4]).astype(int):
            table = np.ascontiguousarray(tables[ch], np.float64)
            info = so.flake_table(table)
            for i in np.flatnonzero(rows[:, 4] == ch):
                iv = tri.beam_intervals(table, info, ang[i, 0], ang[i, 1], d[i])
                _, slots, _, _ = tri.occlusion_dict(ang[i], iv, d[i], rti.BD)
                n_hit[i], most[i] = iv.shape[0], int(slots.max()) if slots.size else 0
        built = want >= 0
        assert np.array_equal(n_hit[built], want[built]), "a constructed beam does not meet the flakes it was built to meet"
        refs.append(dict(rows=rows, tables=tables, bd=rti.BD, n_hit=n_hit, most=most, aug=so.augment(rows, tables, rti.BD, trt.ORDER, thr_poly=np.array(rti.POLY))))
        n_hit_all.append(n_hit); most_all.append(most)
    rows = np.concatenate([r["rows"] for r in refs])
    off = np.concatenate(([0], np.cumsum([r["rows"].shape[0] for r in refs]))).astype(np.int64)
    n_hit, most = np.concatenate(n_hit_all), np.concatenate(most_all)
    # the regions' runs: a (frame, channel) segment queues its beams with 1 .. FRONT_MAX flakes from the front, with more (up to 4) from the back
    runs = {}
    for f, r in enumerate(refs):
        for ch in np.unique(r["rows"][:, 4]).astype(int):
            nh = r["n_hit"][r["rows"][:, 4] == ch]
            runs[(f, ch)] = (int(((nh >= 1) & (nh <= FRONT_MAX)).sum()), int(((nh > FRONT_MAX) & (nh <= 4)).sum()))
    return dict(refs=refs, rows=rows, off=off, runs=runs, pop=rti.class_populations(n_hit), redo=rti.redo_count(n_hit, most), n_hit=n_hit, most=most)


def batch(dtype, scale=1.0):
    return _batch(np.dtype(dtype).name, scale)


def _print_runs(b, what):
    """the back runs the kernel under test is given: the constructed regions one by one, the ordinary channels' summed"""
    built = {(f, ch) for f, runs in enumerate((BACK_RUNS, BACK_RUNS_1)) for ch in runs} | {(0, ch) for ch in SEAM}
    mine = {f"{f}/{int(ch)}": v[1] for (f, ch), v in b["runs"].items() if (f, int(ch)) in built}
    rest = [v[1] for (f, ch), v in b["runs"].items() if (f, int(ch)) not in built and v[1]]
    in_back = (b["n_hit"] > FRONT_MAX) & (b["n_hit"] <= 4)
    print(f"{what}: {b['rows'].shape[0]} rows; beams by flakes met 1..4: {[int((b['n_hit'] == k).sum()) for k in (1, 2, 3, 4)]}; back-run slots by "
          f"frame/channel: {mine}, and {sum(rest)} in {len(rest)} ordinary regions; most slots of one owner in a back run: {int(b['most'][in_back].max())}")


def test_the_batch_holds_the_back_runs_it_claims():
    for dtype in DTYPES:
        b = batch(dtype)
        _print_runs(b, np.dtype(dtype).name)
        for ch, want in BACK_RUNS.items():
            assert b["runs"][(0, ch)] == (FRONT_RUN, want), (ch, b["runs"][(0, ch)])
        for ch, want in BACK_RUNS_1.items():
            assert b["runs"][(1, ch)] == (FRONT_RUN, want), (ch, b["runs"][(1, ch)])
        for ch, (_, m, _) in SEAM.items():
            assert b["runs"][(0, ch)] == (0, 1), ch
        in_back = (b["n_hit"] > FRONT_MAX) & (b["n_hit"] <= 4)
        assert (b["n_hit"][in_back] == 3).sum() > 100 and (b["n_hit"][in_back] == 4).sum() > 100
        assert b["most"][in_back].max() == 7                          # umbrella(3): what a table can give a four-flake beam (module docstring)
        assert all(rows.shape[0] <= 64 * 128 for rows in (r["rows"] for r in b["refs"]))


def _check_compact(b, got, st, what):
    o, s, c, t, _ = got
    for f, ref in enumerate(b["refs"]):
        a = int(b["off"][f])
        trt._check_rows(ref, (o[a:], s[a:], c[f:], t[f:], None), (what, f))
    assert st[0] == 0 and st[2:6].tolist() == b["pop"] and st[6] == b["redo"], (what, st)


@pytest.mark.parametrize("exact", [False, True], ids=["default", "exact"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_compact_entry_against_the_oracle(dtype, exact):
    from lidar_snow_sim_amd import engine
    b = batch(dtype)
    _print_runs(b, f"compact {np.dtype(dtype).name} exact={exact}")
    e = engine.Engine(0)
    try:
        if exact:
            e.ctx.set_exact_math(True)
        tids = [e.table_ids_from_arrays(r["tables"], trt.ORDER) for r in b["refs"]]
        res = []
        for _ in range(2):                                            # twice: the second call finds every buffer in place, same bytes
            got = e.ctx.augment_batch(b["rows"], b["off"], tids, rti.BD, thr_poly=[rti.POLY] * len(tids))
            st = e.ctx.last_status().copy()
            _check_compact(b, got, st, ("compact", np.dtype(dtype).name, exact))
            res.append([np.array(x) for x in got[:4]])
    finally:
        e.ctx.close()
    for f in range(len(b["refs"])):
        a, m = int(b["off"][f]), int(res[0][2][f])
        assert res[0][0][a:a + m].tobytes() == res[1][0][a:a + m].tobytes() and np.array_equal(res[0][1][a:a + m], res[1][1][a:a + m])
    assert np.array_equal(res[0][2], res[1][2]) and np.array_equal(res[0][3], res[1][3])


class _Aligned:
    """the device buffers of one aligned call over a batch's shape"""

    def __init__(self, e, b, dtype):
        dev = torch.device("cuda:0")
        self.e, self.dtype, self.n, self.nf = e, dtype, b["rows"].shape[0], len(b["refs"])
        self.max_frame = int(np.diff(b["off"]).max())
        self.rows = torch.from_numpy(np.array(b["rows"])).to(dev)
        self.off = torch.from_numpy(b["off"]).to(dev)
        self.tids = torch.tensor([e.table_ids_from_arrays(r["tables"], trt.ORDER) for r in b["refs"]], dtype=torch.int32, device=dev)
        self.thr = torch.tensor([rti.POLY] * self.nf, dtype=torch.float64, device=dev)
        self.out = torch.zeros_like(self.rows)
        self.keep = torch.zeros(self.n, dtype=torch.uint8, device=dev)
        self.cnt = torch.zeros(self.nf, dtype=torch.int64, device=dev)
        self.st = torch.zeros(self.nf, 3, dtype=torch.int64, device=dev)
        self.status = torch.zeros(8, dtype=torch.int32, device=dev)
        self.stream = torch.cuda.Stream()

    def call(self):
        self.e.ctx.augment_batch_device_aligned(self.nf, self.n, self.max_frame, self.off.data_ptr(), self.rows.data_ptr(), 0 if self.dtype == np.float32 else 1,
                                                self.tids.data_ptr(), rti.BD, self.thr.data_ptr(), 0, 0.7, 0, self.out.data_ptr(), self.keep.data_ptr(),
                                                self.cnt.data_ptr(), self.st.data_ptr(), 0, self.status.data_ptr(), self.stream.cuda_stream)

    def outputs(self):
        return (self.out, self.keep, self.cnt, self.st, self.status)

    def check(self, b, what):
        """rows in input order with a keep mask: the kept rows are the oracle's, byte for byte from the intensity on"""
        out, keep, cnt, st, status = (t.cpu().numpy() for t in self.outputs())
        assert status[:7].tolist() == [0, -1] + b["pop"] + [b["redo"]], (what, status)
        for f, ref in enumerate(b["refs"]):
            a, z = int(b["off"][f]), int(b["off"][f + 1])
            r_stats, r_aug, r_src = ref["aug"]
            kept = keep[a:z].astype(bool)
            assert int(cnt[f]) == r_src.shape[0] and tuple(int(v) for v in st[f]) == tuple(int(v) for v in r_stats), (what, f)
            assert np.array_equal(np.flatnonzero(kept), np.sort(r_src)), (what, f)
            o = out[a:z][np.sort(r_src)]
            want = r_aug[np.argsort(r_src, kind="stable")]
            assert np.array_equal(o[:, 3:], want[:, 3:]), (what, f)
            np.testing.assert_allclose(o[:, :3], want[:, :3], rtol=1e-6 if self.dtype == np.float32 else 1e-12, atol=0)


@pytest.mark.parametrize("exact", [False, True], ids=["default", "exact"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_aligned_entry_against_the_oracle(dtype, exact):
    from lidar_snow_sim_amd import engine
    b = batch(dtype)
    _print_runs(b, f"aligned {np.dtype(dtype).name} exact={exact}")
    e = engine.Engine(0)
    try:
        if exact:
            e.ctx.set_exact_math(True)
        al = _Aligned(e, b, dtype)
        with torch.cuda.stream(al.stream):
            al.call()
            al.stream.synchronize()
        al.check(b, ("aligned", np.dtype(dtype).name, exact))
    finally:
        e.ctx.close()


def test_graph_capture_replayed_on_changed_input():
    """the aligned call captured once; replayed on the batch it was captured with, then on rows whose beams are a tenth shorter (54 m: still
    beyond every constructed flake, so the same runs with other ranges, amplitudes and maxima) -- each replay against the oracle"""
    from lidar_snow_sim_amd import engine
    dtype = np.float32
    b, b2 = batch(dtype), batch(dtype, 0.9)
    assert b["runs"] != {} and np.array_equal(b["off"], b2["off"]) and b["rows"].tobytes() != b2["rows"].tobytes()
    _print_runs(b, "graph, first input")
    _print_runs(b2, "graph, second input")
    e = engine.Engine(0)
    try:
        al = _Aligned(e, b, dtype)
        rows2 = torch.from_numpy(np.array(b2["rows"])).to(al.rows.device)
        with torch.cuda.stream(al.stream):
            al.call()
            al.call()                                                 # (the second call allocates nothing)
            al.stream.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=al.stream):
                al.call()
            for k, (bb, src) in enumerate(((b, None), (b2, rows2))):
                if src is not None:
                    al.rows.copy_(src)
                for t in al.outputs():
                    t.zero_()
                g.replay()
                al.stream.synchronize()
                al.check(bb, ("replay", k))
    finally:
        e.ctx.close()
