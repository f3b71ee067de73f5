"""CPU: the inputs of tests/test_gpu_aligned_mask.py (tests/aligned_mask_inputs.py) are what the GPU tests take them for, on any machine:
the masks leave the present counts the tests claim, the pre-crop sweep and the narrow calibration put both flag values on more than
1 000 rows and at most 8 rows near an image edge or depth 0, and the fused-chain frames fall on both sides of the 1 000-ground-row rule."""
import numpy as np

import aligned_mask_inputs as ami


def test_ragged_masks_are_bernoulli_draws_that_leave_both_kinds_of_row():
    frames, masks = ami.ragged_frames(), ami.ragged_masks()
    assert [len(f) for f in frames] == [16384, 8192, 16384] == [len(m) for m in masks]
    assert np.any(np.diff(frames[1][:, 4]) < 0) and not np.any(np.diff(frames[0][:, 4]) < 0)      # the middle frame is in firing order
    for m in masks:
        assert 0.68 < m.mean() < 0.72
    assert all(np.array_equal(a, b) for a, b in zip(masks, ami.ragged_masks()))                   # fixed seed


def test_edge_batch_present_counts():
    frames, masks = ami.edge_batch()
    assert len(frames) == len(masks) == len(ami.EDGE_NAMES)
    assert [len(f) for f in frames] == [5000, 5000, 5000, 1025, 2000, 2000, 0, 4096] == [len(m) for m in masks]
    assert tuple(int(m.sum()) for m in masks) == ami.EDGE_PRESENT == (1023, 1024, 1025, 1, 2000, 0, 0, 128)
    assert np.any(np.diff(frames[0][:, 4]) < 0)                                                  # firing order
    assert np.flatnonzero(masks[3]).tolist() == [1024]                                           # only the last row, in the second tile
    assert set(np.flatnonzero(masks[7]) % 64) == {0, 63}
    for k in range(3):                                                                            # present rows in every tile of the 5 000
        assert set(np.flatnonzero(masks[k]) // 1024) == {0, 1, 2, 3, 4}


def test_switch_masks_lie_on_the_claimed_sides_of_two_to_the_19():
    n = 20 * 32768
    assert n == 655360 > (1 << 19)
    half = sum(int(m.sum()) for m in ami.switch_masks("half"))
    dense = sum(int(m.sum()) for m in ami.switch_masks("dense"))
    assert 300000 < half < (1 << 19) < dense < n, (half, dense)


def test_precrop_sweep_under_the_narrow_camera():
    pc = ami.precrop_sweep()
    assert pc.shape == (64 * 512, 5)
    flag, decided = ami.fov_reference(pc)
    assert int(flag.sum()) >= 1000 and int((~flag).sum()) >= 1000, (int(flag.sum()), int((~flag).sum()))
    assert int((~decided).sum()) <= 8, int((~decided).sum())


def test_fused_frames_fall_on_both_sides_of_the_ground_row_rule():
    frames, masks = ami.fused_frames()
    ground = [ami.present_ground_rows(f, m) for f, m in zip(frames, masks)]
    assert ground[0] > 1000 and ground[1] > 1000 and ground[2] < 1000, ground
