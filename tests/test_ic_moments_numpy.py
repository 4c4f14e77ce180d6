"""A numpy IC_Angle that returns the integer moments themselves, the comparator
of tests/test_describe_rows_gpu.py, pinned here against the oracle: fed
through the numpy fastAtan2 restatement it reproduces the oracle's angle for
every keypoint of one extracted frame.

moments_np sums over the circular patch as a mask, not row by row or column
by column: m01 = sum v I(u, v), m10 = sum u I(u, v) over |v| <= 15,
|u| <= umax[|v|] (src/ORBextractor.cc:127-152).
"""
import numpy as np

from orb_slam_amd import synth
from oracle_lib import RefExtractor
from test_cv24_numpy import fast_atan2_np
from test_orb_numpy import umax_np

HP = 15      # HALF_PATCH_SIZE
EDGE = 16    # the padded level's border


def circle_mask(umax):
    """inside[v + 15, u + 15] of the circular patch."""
    a = np.arange(-HP, HP + 1)
    return np.abs(a)[None, :] <= np.asarray(umax)[np.abs(a)][:, None]


def moments_np(padded, x, y, umax):
    """(m01, m10) at level position (x, y) of a padded level."""
    a = np.arange(-HP, HP + 1)
    cy, cx = EDGE + int(y), EDGE + int(x)
    win = padded[cy - HP:cy + HP + 1, cx - HP:cx + HP + 1].astype(np.int64) * circle_mask(umax)
    return int((win * a[:, None]).sum()), int((win * a[None, :]).sum())


def angle_np(m01, m10):
    return fast_atan2_np(np.array([m01], np.float32), np.array([m10], np.float32))[0]


def test_moments_reproduce_oracle_angles():
    umax = umax_np()
    mask = circle_mask(umax)
    assert mask.shape == (31, 31) and mask[15].all() and mask[:, 15].all() and not mask[0, 0]
    assert int(mask.sum()) == int((2 * umax + 1).sum() * 2 - (2 * umax[0] + 1))
    ex = RefExtractor(300)
    kps, _ = ex(synth.noise_frame(160, 128, 21))
    assert np.array_equal(umax, ex.umax()[:HP + 1])
    at = 0
    for lvl in range(8):
        lk = ex.level_keys(lvl)
        raw = ex.level(lvl)
        for k in range(len(lk)):
            m01, m10 = moments_np(raw, lk["x"][k], lk["y"][k], umax)
            assert angle_np(m01, m10) == lk["angle"][k] == kps["angle"][at + k], (lvl, k, m01, m10)
        at += len(lk)
    assert at == len(kps) and at > 200
