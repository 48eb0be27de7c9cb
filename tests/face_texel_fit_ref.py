"""fp64 numpy restatement of K36 (tp_face_texel_shade_bwd), of its 64-bit fixed-point scheme and of FaceTexelFitter's conjugate-gradient
loop, written from the contract in include/texpose_amd.h (not from the kernel or the module), with the figures the tests pin."""
import numpy as np

from face_texels_ref import node, texel_count

FIXED_BITS = 36


def cell(face, verts, faces, pose, intr, H, W, R):
    """K35's per-pixel cell -> slots [B,H,W,3] int64 (within the face's T texels), weights [B,H,W,3] float64, valid [B,H,W] bool.
    Invalid pixels (every rule by which K35 writes zeros except the one on the colour's value) carry slot 0 and weight 0."""
    face = np.asarray(face).reshape(-1, H, W)
    B = face.shape[0]
    verts = np.asarray(verts, dtype=np.float64)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    pose = np.asarray(pose, dtype=np.float64).reshape(B, 3, 4)
    intr = np.broadcast_to(np.asarray(intr, dtype=np.float64), (B, 3, 3))
    V, F = len(verts), len(faces)
    slots, weights, valid = np.zeros((B, H, W, 3), np.int64), np.zeros((B, H, W, 3)), np.zeros((B, H, W), bool)
    ii, jj = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    with np.errstate(all="ignore"):
        for b in range(B):
            fb_ = face[b].astype(np.int64)
            ok = (fb_ >= 0) & (fb_ < F)
            vi = faces[np.where(ok, fb_, 0)]
            ok &= ((vi >= 0) & (vi < V)).all(-1)
            X = verts[np.clip(vi, 0, V - 1)]
            P, K = pose[b], intr[b]
            c = [P[r, 0] * X[..., 0] + P[r, 1] * X[..., 1] + P[r, 2] * X[..., 2] + P[r, 3] for r in range(3)]
            ok &= ((c[2] > 0) & np.isfinite(c[0]) & np.isfinite(c[1]) & np.isfinite(c[2])).all(-1)
            q = [K[r, 0] * c[0] + K[r, 1] * c[1] + K[r, 2] * c[2] for r in range(3)]
            u, v, iz = q[0] / q[2], q[1] / q[2], 1.0 / c[2]
            area = (u[..., 1] - u[..., 0]) * (v[..., 2] - v[..., 0]) - (v[..., 1] - v[..., 0]) * (u[..., 2] - u[..., 0])
            ok &= np.isfinite(area) & (np.abs(area) > 1e-10)
            px, py = jj + 0.5, ii + 0.5
            t = []
            for k in range(3):
                s, e = (k + 1) % 3, (k + 2) % 3
                t.append((((u[..., e] - u[..., s]) * (py - v[..., s]) - (v[..., e] - v[..., s]) * (px - u[..., s])) / area) * iz[..., k])
            tot = (t[0] + t[1]) + t[2]
            w = [np.where(tk / tot < 0, 0.0, tk / tot) for tk in t]
            s2 = (w[0] + w[1]) + w[2]
            w = [wk / s2 for wk in w]
            ok &= np.isfinite(w[0]) & np.isfinite(w[1]) & np.isfinite(w[2])
            w = [np.where(ok, wk, 0.0) for wk in w]
            a, bb = R * w[1], R * w[2]
            ci = np.minimum(np.floor(a).astype(np.int64), R - 1)
            cj = np.minimum(np.floor(bb).astype(np.int64), R - 1 - ci)
            fa, fb = a - ci, bb - cj
            upper = (fa + fb > 1.0) & (ci + cj <= R - 2)
            n = np.stack([np.where(upper, node(ci + 1, cj + 1, R), node(ci, cj, R)), node(ci + 1, cj, R), node(ci, cj + 1, R)], -1)
            ww = np.stack([np.where(upper, (fa + fb) - 1.0, (1.0 - fa) - fb), np.where(upper, 1.0 - fb, fa), np.where(upper, 1.0 - fa, fb)], -1)
            slots[b], weights[b], valid[b] = np.where(ok[..., None], n, 0), np.where(ok[..., None], ww, 0.0), ok
    return slots, weights, valid


def contributions(face, verts, faces, grad_rgb, pose, intr, H, W, R, node_index=None, U=None):
    """The flat list of what the adjoint adds: destinations [M], weights [M] float64, gradients [M,3] float64 (the pixel's grad_rgb) and
    the number of destinations N -- one entry per (contributing pixel, slot) whose destination exists."""
    slots, weights, valid = cell(face, verts, faces, pose, intr, H, W, R)
    T = texel_count(R)
    g = np.asarray(grad_rgb).reshape(valid.shape + (3,))
    with np.errstate(all="ignore"):
        valid = valid & np.isfinite(g).all(-1)
    f = np.asarray(face).reshape(valid.shape).astype(np.int64)[valid]
    dest = f[:, None] * T + slots[valid]                                     # [P,3]
    w, gp = weights[valid], g[valid].astype(np.float64)
    N = len(np.asarray(faces).reshape(-1, 3)) * T
    keep = np.ones(dest.shape, bool)
    if node_index is not None:
        dest = np.asarray(node_index, dtype=np.int64).reshape(-1)[dest]
        N = int(U)
        keep = (dest >= 0) & (dest < N)
    return dest[keep], w[keep], np.repeat(gp[:, None], 3, 1)[keep], N


def shade_bwd(face, verts, faces, grad_rgb, pose, intr, H, W, R, node_index=None, U=None):
    """The exact adjoint in fp64 -> dict(grad [N,3], weight [N], count [N] = n_d, gmax: the largest |grad_rgb| component over the
    contributing pixels, as a float)."""
    dest, w, g, N = contributions(face, verts, faces, grad_rgb, pose, intr, H, W, R, node_index, U)
    grad = np.stack([np.bincount(dest, w * g[:, c], N) for c in range(3)], -1) if len(dest) else np.zeros((N, 3))
    return dict(grad=grad, weight=np.bincount(dest, w, N), count=np.bincount(dest, minlength=N),
                gmax=float(np.abs(g).max()) if len(dest) else 0.0)


def gmax_exponent(gmax):
    """e = max(floor(log2 gmax), -126); -126 for zero"""
    return max(int(np.frexp(np.float32(gmax))[1]) - 1, -126) if gmax > 0 else -126


def shade_bwd_fixed(face, verts, faces, grad_rgb, pose, intr, H, W, R, node_index=None, U=None):
    """The fixed-point scheme emulated in int64 (np.rint rounds to nearest even) -> dict(grad [N,3] float32, weight [N] float32)."""
    dest, w, g, N = contributions(face, verts, faces, grad_rgb, pose, intr, H, W, R, node_index, U)
    e = gmax_exponent(float(np.abs(g).max()) if len(dest) else 0.0)
    acc, wacc = np.zeros((N, 3), np.int64), np.zeros(N, np.int64)
    for c in range(3):
        np.add.at(acc[:, c], dest, np.rint((w * g[:, c]) * 2.0 ** (FIXED_BITS - e)).astype(np.int64))
    np.add.at(wacc, dest, np.rint(w * 2.0 ** FIXED_BITS).astype(np.int64))
    return dict(grad=(acc.astype(np.float64) * 2.0 ** (e - FIXED_BITS)).astype(np.float32),
                weight=(wacc.astype(np.float64) * 2.0 ** -FIXED_BITS).astype(np.float32))


class Views:
    """The stored views of a fit as one sparse S: per contributing pixel three destinations and weights (node_index applied)."""

    def __init__(self, face, verts, faces, pose, intr, H, W, R, node_index, U, rgb, weight):
        slots, weights, valid = cell(face, verts, faces, pose, intr, H, W, R)
        f = np.asarray(face).reshape(valid.shape).astype(np.int64)[valid]
        self.dest = np.asarray(node_index, dtype=np.int64).reshape(-1)[f[:, None] * texel_count(R) + slots[valid]]
        self.w, self.valid, self.U = weights[valid], valid, int(U)
        self.rgb = np.asarray(rgb, dtype=np.float64).reshape(valid.shape + (3,))[valid]
        self.m = np.asarray(weight, dtype=np.float64).reshape(valid.shape)[valid]

    def shade(self, x):
        return (self.w[..., None] * x[self.dest]).sum(1)

    def adjoint(self, g):
        v = self.w[..., None] * g[:, None, :]
        return np.stack([np.bincount(self.dest.reshape(-1), v[..., c].reshape(-1), self.U) for c in range(3)], -1)

    def coverage(self):
        return np.bincount(self.dest.reshape(-1), self.w.reshape(-1), self.U)


def inner_coverage(face, F):
    """pixels that hold a face and whose four neighbours do"""
    c = (np.asarray(face) >= 0) & (np.asarray(face) < F)
    inner = np.zeros_like(c)
    inner[:, 1:-1, 1:-1] = c[:, 1:-1, 1:-1] & c[:, :-2, 1:-1] & c[:, 2:, 1:-1] & c[:, 1:-1, :-2] & c[:, 1:-1, 2:]
    return inner


def pcg(x, r, m_inv, apply, after_step, iters, dtype=np.float64):
    """``iters`` steps of preconditioned conjugate gradients from x, whose residual b - A x is r: ``apply(p)`` is A p, ``m_inv`` the inverse
    of the diagonal preconditioner, ``after_step(x)`` is called after every step -> x.  The vectors are ``dtype``, the scalars fp64."""
    dot = lambda a, b: float((a.astype(np.float64) * b.astype(np.float64)).sum())
    z = r * m_inv
    p, rz = z.copy(), dot(r, z)
    for _ in range(iters):
        ap = apply(p)
        pap = dot(p, ap)
        alpha = rz / pap if pap > 0 else 0.0
        x, r = x + dtype(alpha) * p, r - dtype(alpha) * ap
        z = r * m_inv
        rz_new = dot(r, z)
        beta = rz_new / rz if rz > 0 else 0.0
        p, rz = z + dtype(beta) * p, rz_new
        after_step(x)
    return x


def fit_loop(views, prior, start, lam, iters, dtype=np.float64):
    """FaceTexelFitter.fit: ``iters`` steps of conjugate gradients on (S^T m S + lam) x = S^T m I + lam prior, preconditioned with
    coverage + lam -> dict(nodes, coverage, rms [iters + 1]).  ``dtype``: the precision of the vectors (the scalars stay fp64)."""
    x, prior = np.array(start, dtype=dtype), np.asarray(prior, dtype=dtype)
    S = lambda v: views.shade(v.astype(np.float64)).astype(dtype)
    St = lambda g: views.adjoint(g.astype(np.float64)).astype(dtype)
    m, total = views.m.astype(dtype)[:, None], float(views.m.sum())
    rms_of = lambda v: float(np.sqrt((views.m[:, None] * (S(v).astype(np.float64) - views.rgb) ** 2).sum() / (3.0 * total)))
    coverage = views.coverage()
    m_inv = (1.0 / (coverage[:, None] + lam)).astype(dtype)
    r = St(m * (views.rgb.astype(dtype) - S(x))) + dtype(lam) * (prior - x)
    rms = [rms_of(x)]
    x = pcg(x, r, m_inv, lambda p: St(m * S(p)) + dtype(lam) * p, lambda v: rms.append(rms_of(v)), iters, dtype)
    return dict(nodes=x, coverage=coverage, rms=np.array(rms))


def psnr(img, want, mask):
    return 10 * np.log10(1.0 / ((np.asarray(img, np.float64) - np.asarray(want, np.float64))[mask] ** 2).mean())


# ---- measured by tests/test_face_texel_fit_cpu.py with this file's loop (fp64), pinned there
# The round trip of tests/test_face_texels_cpu.py (sphere uv_sphere(12, 16), 14 Fibonacci views, 96 x 96, f = 300, analytic colour of 3 mm
# period, held-out view sphere_view_poses(5, 400)[1]); lam = 0.1, 4 iterations from the bake, the default weights (inner pixels):
#   R: (held-out PSNR of the bake, of the fit, training rms of the bake, of the fit)
ROUND_TRIP = {4: (27.34, 34.14, 0.0410, 0.01844), 8: (35.94, 47.04, 0.0154, 0.00375)}       # (8: 36 of 11,520 nodes stay on the prior)
# the same shrunk to 64 x 64, f = 200, R = 4 (the device test's case)
ROUND_TRIP_SMALL = {4: (26.05, 34.10, 0.0478, 0.01820)}                                            # (5 nodes stay on the prior)
# The consistent system: sphere, 14 views, 64 x 64, f = 200, R = 2, photographs S x* for x* = RandomState(11).rand(U, 3), lam = 1e-6,
# prior 0.5, from zeros, 32 iterations: max |x - x*| over the nodes with coverage >= 1 -- with fp64 vectors and with fp32 vectors
CONSISTENT_ERROR = 1.39e-6                      # 767 of 768 nodes have coverage >= 1; training rms 0.545 -> 1.9e-8
CONSISTENT_ERROR_FP32 = 1.46e-6                 # below 4 x 1.39e-6 + 1e-4, the device test's bar
