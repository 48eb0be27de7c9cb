"""The Visible Surface Discrepancy of DESIGN section 16 (kernel K26 `tp_vsd`), said again in numpy fp64 -- written from the rules in
include/texpose_amd.h, independent of texpose_amd/pose_error.py.  Not a test module.

Besides the counts and the errors, `vsd_ref` returns per pose pair the number of NEAR-TIES: (pixel, comparison) pairs whose fp64
margin to the decision is below `TIE_MM` -- `D - D_test` against `delta` for the two visibility tests of a pixel, `|D_gt - D_est|`
against every `tau` on a pixel both models cover.  Two correct fp64 evaluations may decide such a pair differently (a different but
equally valid rounding of f), every other pair they must decide alike; so a count of an implementation under test may differ from
the helper's by at most this number."""
import numpy as np

TIE_MM = 1e-9


def vsd_ref(z_est, z_gt, depth_test, intr, tau_mm, delta_mm=15.0, frame=None):
    """z_est, z_gt [B,H,W] float32, depth_test [Ft,H,W] float32, intr [B,3,3] or [3,3], tau_mm [B,T] float32, frame [B] or None
    -> dict(counts [B,2+T] int64, err [B,T] float32, err64 [B,T] float64, near_ties [B] int64)."""
    z_est, z_gt, depth_test = (np.asarray(a, dtype=np.float32) for a in (z_est, z_gt, depth_test))
    tau_mm = np.asarray(tau_mm, dtype=np.float32)
    B, H, W = z_est.shape
    Ft, T = depth_test.shape[0], tau_mm.shape[1]
    intr = np.broadcast_to(np.asarray(intr, dtype=np.float32), (B, 3, 3)).astype(np.float64)
    delta = float(np.float32(delta_mm))
    counts = np.zeros((B, 2 + T), dtype=np.int64)
    err64 = np.ones((B, T), dtype=np.float64)
    ties = np.zeros(B, dtype=np.int64)
    jj = np.arange(W, dtype=np.float64)[None, :]
    ii = np.arange(H, dtype=np.float64)[:, None]
    for b in range(B):
        if frame is not None:
            fr = min(max(int(frame[b]), 0), Ft - 1)
        else:
            assert Ft in (1, B)
            fr = 0 if Ft == 1 else b
        fx, cx, fy, cy = intr[b, 0, 0], intr[b, 0, 2], intr[b, 1, 1], intr[b, 1, 2]
        u = ((jj + 0.5) - cx) / fx
        v = ((ii + 0.5) - cy) / fy
        f = np.sqrt((u * u + v * v) + 1.0)
        ze, zg, dt = z_est[b], z_gt[b], depth_test[fr]
        with np.errstate(invalid="ignore"):
            ok_e, ok_g, missing = ze > 0, zg > 0, ~(dt > 0)
            De, Dg, Dt = ze.astype(np.float64) * f, zg.astype(np.float64) * f, dt.astype(np.float64) * f
            m_g, m_e = (Dg - Dt) - delta, (De - Dt) - delta
            vis_g = ok_g & (missing | (Dg - Dt <= delta))
            vis_e = ok_e & (missing | (De - Dt <= delta) | vis_g)
            inter = vis_g & vis_e
            diff = np.abs(Dg - De)
            # the visibility comparisons that are evaluated and matter: a model pixel with a measured depth
            ties[b] += np.count_nonzero(ok_g & ~missing & (np.abs(m_g) < TIE_MM)) + np.count_nonzero(ok_e & ~missing & (np.abs(m_e) < TIE_MM))
            counts[b, 0], counts[b, 1] = np.count_nonzero(vis_g | vis_e), np.count_nonzero(inter)
            for t in range(T):
                tau = float(tau_mm[b, t])
                counts[b, 2 + t] = np.count_nonzero(inter & (diff >= tau))
                ties[b] += np.count_nonzero(ok_e & ok_g & (np.abs(diff - tau) < TIE_MM))
        n_u, n_i = counts[b, 0], counts[b, 1]
        if n_u > 0:
            err64[b] = (counts[b, 2:] + n_u - n_i).astype(np.float64) / float(n_u)
    return dict(counts=counts, err=err64.astype(np.float32), err64=err64, near_ties=ties)
