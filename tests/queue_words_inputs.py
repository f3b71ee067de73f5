"""Input of tests/test_gpu_queue_words.py that tests/row_tier_inputs.py lacks, made on any machine (NumPy only): the frame `crowd`.

The dict queue of the pass over all rows (csrc/sg_queue.h) is cut into regions -- one per (frame, channel) segment --, and a region's beams
with few flakes fill its slice from the front, the others from the back; k_power_few / k_power take them in items of up to 64 slots.  The
frames of row_tier_inputs put three ordinary beams on a channel, so no region of theirs queues more than a handful.  Here channel
CROWD_CHANNEL carries CROWD_BEAMS ordinary beams of 40 .. 119 m against its fixture table: more than 64 beams with one flake (the front run
crosses a group of 64 slots whatever the few-flake limit, 1 .. 3, is), beams with three and four flakes (back-filled slots for every such
limit, and for the capacities 8 and 16 too), beams with five to seven (the 8-entry tier), and front and back runs that are no multiple of 64
(an item that does not fill its wave).  The other channels carry three ordinary beams each, as in row_tier_inputs.  tests/test_queue_words.py shows on the CPU, from the
oracle alone, that these populations exist, and asserts the status words the GPU test compares with."""
from functools import lru_cache

import numpy as np

import row_tier_inputs as rti

CROWD_CHANNEL = 5
CROWD_BEAMS = 400
# capacity of the pass over all rows -> status words [2 .. 5] (beams per later tier) and [6] (beams the row kernels redo); the same for float32
# and float64 rows.  tests/test_queue_words.py derives them from the oracle's intersecting counts and asserts these literals.
EXPECTED = {4: ([44, 0, 0, 0], 0), 8: ([0, 0, 0, 0], 0), 16: ([0, 0, 0, 0], 0)}


@lru_cache(maxsize=None)
def _crowd(dtype_name):
    dtype = np.dtype(dtype_name).type
    rng = np.random.default_rng(8201)
    fix = rti.fixture_tables()
    tables = [fix[c % 4] for c in range(rti.N_LASERS)]
    az_c, d_c, ch_c = rti._ordinary(rng, [CROWD_CHANNEL], CROWD_BEAMS, 40.0, 119.0)
    others = [c for c in range(rti.N_LASERS) if c != CROWD_CHANNEL]
    az_o, d_o, ch_o = rti._ordinary(rng, others, 3, 3.0, 119.0)
    az, d, ch = np.concatenate((az_c, az_o)), np.concatenate((d_c, d_o)), np.concatenate((ch_c, ch_o))
    o = np.argsort(ch, kind="stable")                                # channel-major
    rows = rti._rows(az[o], d[o], ch[o], rng, dtype)
    rows.setflags(write=False)
    return dict(rows=rows, tables=tables, groups={}, bd=rti.BD)


def crowd(dtype=np.float32):
    """dict(rows, tables, groups, bd), read-only -- the shape of row_tier_inputs.frames()[name]"""
    return _crowd(np.dtype(dtype).name)
