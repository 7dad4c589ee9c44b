"""The staged round trip that the PnP and the two-view calls share (LpStagedCall, csrc/api.hip) across calls of
different kinds on ONE fresh context: its page-locked block does not exist at the first call and has to grow inside this test, then
serves calls that deliver under another arrival counter.  Every result is compared with its *_host form byte for byte, as in
tests/test_pnp_gpu.py and tests/test_two_view_gpu.py; those files cross neither growth nor a change of counter on purpose.

  1  pnp_ransac_batch       S1, 1 iteration        the block is made (13 KB needed, 20 KB made)
  2  two_view_ransac_batch  S8, 100 iterations     the block grows (about 72 KB needed), counter LP_DONE_TWO_VIEW
  3  two_view_check_poses   P = 8, n = 65          fits, same counter
  -  pnp_ransac_batch       0 iterations           refused: nothing staged, nothing armed
  4  pnp_ransac_batch       S11, 100 iterations    the block grows again (about 155 KB needed), counter LP_DONE_PNP
  5  pnp_ransac_batch       S1, 1 iteration        call 1 again, in the grown block"""
import numpy as np
import pytest

import pnp_cases as P
import two_view_cases as T

pytestmark = pytest.mark.gpu


def _bytes(arrays):
    return [a.tobytes() for a in arrays]


def test_growth_then_reuse_under_another_counter(hiplib):
    from lpslam_amd import _build
    _build.host_library()
    pnp, tv = P.batches(), T.batches()
    s1, s11, t8 = P.concat(pnp["S1"]), P.concat(pnp["S11"]), T.concat(tv["S8"])
    scene = T.general(65, 2)
    t = scene["t"] / np.linalg.norm(scene["t"])
    R8 = np.stack([scene["R"]] * 2 + [T.rot([0.3 * k, 1.0, -0.2], 0.05 * k) @ scene["R"] for k in range(1, 7)])
    t8v = np.stack([t, -t] + [T.rot([1.0, 0.1 * k, 0.4], 0.4 * k) @ t for k in range(1, 7)])
    fl = (np.arange(65) % 3 != 0).astype(np.uint8)
    ctx = hiplib.Context(640, 480, max_keypoints=500, num_levels=2, max_images=2)           # fresh: no page-locked block yet
    try:
        first = hiplib.pnp_ransac_batch(ctx, *s1, P.CAM, 1, P.SEED)
        assert _bytes(first) == _bytes(hiplib.pnp_ransac_batch_host(*s1, P.CAM, 1, P.SEED))
        got = hiplib.two_view_ransac_batch(ctx, *t8, 1.0, 100, T.SEED)
        assert _bytes(got) == _bytes(hiplib.two_view_ransac_batch_host(*t8, 1.0, 100, T.SEED))
        got = hiplib.two_view_check_poses(ctx, R8, t8v, T.K, scene["p1"], scene["p2"], fl, 4.0)
        assert got[0].shape == (8, 65, 3)
        assert _bytes(got) == _bytes(hiplib.two_view_check_poses_host(R8, t8v, T.K, scene["p1"], scene["p2"], fl, 4.0))
        with pytest.raises(hiplib.LpslamHipError):
            hiplib.pnp_ransac_batch(ctx, *s1, P.CAM, 0, P.SEED)
        got = hiplib.pnp_ransac_batch(ctx, *s11, P.CAM, 100, P.SEED)
        assert _bytes(got) == _bytes(hiplib.pnp_ransac_batch_host(*s11, P.CAM, 100, P.SEED))
        again = hiplib.pnp_ransac_batch(ctx, *s1, P.CAM, 1, P.SEED)
        assert _bytes(again) == _bytes(first)
    finally:
        ctx.close()
