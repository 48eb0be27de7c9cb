"""GPU: the two reduction families of the PatchGAN half of a training step against their fp64 restatements (tests/norm_ref.py) at the
edges of their tiling constants: csrc/spectral_norm.hip (kernels A-E through ops.spectral_norm_fwd / _fwd_sets / _bwd) and
csrc/inorm_lrelu.hip (forward, backward, double backward through ops.inorm_lrelu_* and autograd_ops.inorm_lrelu).

Accuracy is the project's fp32 rule (`within_rule` of tests/test_gpu_lab_loss.py), per output tensor:
    e_k <= 2 e_t + floor
e_k: the kernel's largest absolute error against the fp64 restatement; e_t: that of the SAME restatement evaluated by torch in fp32 on
the CPU on the same inputs (no code under test); floor: one fp32 spacing of the largest reference value.

The spectral-norm shapes, one per constant of the kernels (rows x cols):
    (1,1) (1,5) (3,4)            one row / one column / the smallest 16-byte row
    (4,1024) (5,819)             kernel B's four rows per workgroup, full and with a partly filled second workgroup; 4096 / 4095 elements
    (17,241) (63,255) (64,256) (65,257)      kernel A's 64-row slab and 256-column block, one below / at / one above
    (255,36) (256,16) (257,7) (511,9) (512,8)    kernel C's two values of s per thread around row 256, the last slab, 8 slabs
    (2,8192) (2,8196) (3,8193) (1,16384)     32 KB of LDS exactly, just above (vector and scalar path), the 64 KB limit
    (512,4096)                   the largest PatchGAN weight: 512 workgroups of kernel C, 2048 of kernel E
in three calls (BATCHES), each mixing 16-byte and scalar-path weights, with its widest weight (> 8192 columns: the raised LDS limit, the
LDS size shared by the whole launch) not first and narrow weights behind it; the first call has TP_SN_MAX_WEIGHTS weights, the eighth a
(64,256) weight one float into its buffer (4-byte aligned: the scalar path at cols % 4 == 0)."""
import functools

import numpy as np
import pytest
import torch

import norm_ref as R
from test_gpu_lab_loss import within_rule

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
OFFSET = "one float in"                      # marks the weight that is placed at a 4-byte-aligned address
BATCHES = (
    ((1, 1), (1, 5), (1, 16384), (3, 4), (4, 1024), (5, 819), (17, 241), (64, 256, OFFSET)),
    ((63, 255), (2, 8196), (64, 256), (65, 257), (255, 36), (256, 16)),
    ((257, 7), (3, 8193), (511, 9), (512, 8), (2, 8192), (512, 4096)),
)
SCALED = ((65, 257), (512, 8))               # rerun with W 2^+-30: a hidden absolute epsilon would show
MAX_RATIO = {}                               # output name -> largest e_k / e_t seen (printed; the docstrings quote it)


@pytest.fixture(scope="module")
def ops():
    from texpose_amd import ops as _ops
    return _ops


def cu(t):
    return t.to(DEV)


def rule(name, got, want, torch32):
    """`within_rule`, and the largest e_k / e_t per output (the part of `name` before the first blank) for the docstrings."""
    g, w, t = (x.detach().double().cpu().reshape(-1) for x in (got, want, torch32))
    e_k, e_t = float((g - w).abs().max()), float((t - w).abs().max())
    key = name.split(" ")[0]
    MAX_RATIO[key] = max(MAX_RATIO.get(key, 0.0), e_k / e_t if e_t > 0 else (0.0 if e_k == 0 else float("inf")))
    within_rule(name, g, w, t)


@pytest.fixture(scope="module", autouse=True)
def _print_largest_ratios():
    yield
    for k in sorted(MAX_RATIO):
        print("largest e_k / e_t of %-6s %.3f" % (k, MAX_RATIO[k]))


# ------------------------------------------------------------------------------------------ spectral norm
def key_of(shape, scale=0):
    return (shape[0], shape[1], scale)


def place(W, shape):
    """The weight on the device; the OFFSET one as a contiguous view starting one float into a buffer."""
    if len(shape) == 3:
        buf = torch.empty(W.numel() + 1, device=DEV)
        view = buf[1:].view(W.shape)
        view.copy_(W)
        assert view.is_contiguous() and view.data_ptr() % 16 == 4
        return view
    w = cu(W)
    assert w.data_ptr() % 16 == 0
    return w


def start_uv(rows, cols, scale, mode):
    """u, v a call starts from (float32, CPU): the case's random unit vectors; "eval_iterated": what one reference power iteration makes of
    them, rounded -- the state an eval-mode forward meets in practice (sigma = u . W v is then |W v|, not a cancelling sum)."""
    W, u, v = R.sn_case(rows, cols, scale)[:3]
    if mode == "eval_iterated":
        _, u, v, _ = R.sn_forward(W.double(), u.double(), v.double(), True)
    return u.float(), v.float()


def device_inputs(batch, scale=0, mode="train"):
    ws = [place(R.sn_case(*key_of(s, scale))[0], s) for s in batch]
    uv = [start_uv(*key_of(s, scale), mode) for s in batch]
    return ws, [cu(u).clone() for u, _ in uv], [cu(v).clone() for _, v in uv]


@functools.lru_cache(maxsize=None)
def sn_ref(rows, cols, scale, mode, n_sets=1):
    """[(fp64 (W_sn, u, v, sigma), fp32 the same)] per set, from the call's float32 inputs; shared, never written to."""
    W = R.sn_case(rows, cols, scale)[0]
    u, v = start_uv(rows, cols, scale, mode)
    if mode != "train":
        return [(R.sn_forward(W.double(), u.double(), v.double(), False), R.sn_forward(W, u, v, False))]
    return list(zip(R.sn_forward_sets(W.double(), u.double(), v.double(), n_sets), R.sn_forward_sets(W, u, v, n_sets)))


def check_forward(tag, got, ref64, ref32):
    for name, g, a, b in zip(("W_sn", "u", "v", "sigma"), got, ref64, ref32):
        rule("%s %s" % (name, tag), g.reshape(-1), a.reshape(-1), b.reshape(-1))


FORWARD_CALLS = [(BATCHES[0], 0), (BATCHES[1], 0), (BATCHES[2], 0), (SCALED, 30), (SCALED, -30)]


@pytest.mark.parametrize("mode", ["train", "eval", "eval_iterated"])
@pytest.mark.parametrize("call", range(len(FORWARD_CALLS)))
def test_spectral_norm_forward_meets_the_fp32_rule(ops, call, mode):
    """W_sn, u, v and sigma of every weight of a call, training and eval mode; u / v in place (eval: untouched, bit for bit), the keep_uv
    copies equal to them, the `out=` form and the form without copies bit-identical.  Calls 3 and 4: the SCALED shapes with W 2^+-30.
    Largest e_k / e_t on the MI355X over this module's spectral-norm tests (printed behind its last test): W_sn 2.616, u 3.254, v 6.876,
    sigma 7.326 -- the ratios above 2 are errors of one or two fp32 spacings where torch's own is a fraction of one (the floor's case)."""
    batch, scale = FORWARD_CALLS[call]
    training = mode == "train"
    ws, us, vs = device_inputs(batch, scale, mode)
    u0, v0 = [u.clone() for u in us], [v.clone() for v in vs]
    outs, sig, uc, vc = ops.spectral_norm_fwd(ws, us, vs, training, keep_uv=True)
    for i, s in enumerate(batch):
        tag = "%dx%d%s %s 2^%d" % (s[0], s[1], " offset" if len(s) == 3 else "", mode, scale)
        (r64, r32), = sn_ref(*key_of(s, scale), mode)
        check_forward(tag, (outs[i], us[i], vs[i], sig[i]), r64, r32)
        assert torch.equal(uc[i], us[i]) and torch.equal(vc[i], vs[i]), tag
        if not training:
            assert torch.equal(us[i], u0[i]) and torch.equal(vs[i], v0[i]), tag
    # the same into pre-allocated buffers full of garbage, and without the copies
    ws2, us2, vs2 = device_inputs(batch, scale, mode)
    bufs = ops.spectral_norm_buffers(ws2, us2, vs2)
    for group in bufs:
        for t in group:
            t.fill_(float("nan"))
    o2, s2, uc2, vc2 = ops.spectral_norm_fwd(ws2, us2, vs2, training, out=bufs)
    ws3, us3, vs3 = device_inputs(batch, scale, mode)
    o3, s3 = ops.spectral_norm_fwd(ws3, us3, vs3, training)
    for i in range(len(batch)):
        assert o2[i].data_ptr() == bufs[0][i].data_ptr() and s2[i].data_ptr() == bufs[1][i].data_ptr()
        for a, c, d in ((outs[i], o2[i], o3[i]), (sig[i], s2[i], s3[i]), (us[i], us2[i], us3[i]), (vs[i], vs2[i], vs3[i]), (uc[i], uc2[i], us3[i]),
                        (vc[i], vc2[i], vs3[i])):
            assert torch.equal(a, c) and torch.equal(a, d), (batch[i], training)


@pytest.mark.parametrize("n_sets", [1, 2, 3])
@pytest.mark.parametrize("b", range(len(BATCHES)))
def test_spectral_norm_sets_are_the_single_calls_and_meet_the_rule(ops, b, n_sets):
    """tp_sn_fwd_sets with 1, 2 and 3 sets: every set bit-identical to that many tp_sn_fwd calls in a row, and within the rule against the
    reference iterated."""
    batch = BATCHES[b]
    ws, us, vs = device_inputs(batch)
    sets = ops.spectral_norm_fwd_sets(ws, us, vs, n_sets)
    ws1, us1, vs1 = device_inputs(batch)
    singles = [ops.spectral_norm_fwd(ws1, us1, vs1, True, keep_uv=True) for _ in range(n_sets)]
    assert len(sets) == n_sets
    for k in range(n_sets):
        for i, s in enumerate(batch):
            for a, c in zip(sets[k], singles[k]):
                assert torch.equal(a[i], c[i]), (s, k)
            r64, r32 = sn_ref(*key_of(s), "train", n_sets)[k]
            check_forward("%dx%d set %d of %d" % (s[0], s[1], k + 1, n_sets), (sets[k][0][i], sets[k][2][i], sets[k][3][i], sets[k][1][i]), r64, r32)
    for i in range(len(batch)):
        assert torch.equal(us[i], us1[i]) and torch.equal(vs[i], vs1[i]) and torch.equal(us[i], sets[-1][2][i])


@functools.lru_cache(maxsize=None)
def bwd_inputs(rows, cols):
    """Two normalised instances of the weight as the REFERENCE gives them, rounded to float32: the backward kernels and both evaluations
    of the restatement start from the same (W_sn, u, v, sigma) -- [(W_sn, u, v, sigma)] * 2."""
    W, u, v = R.sn_case(rows, cols)[:3]
    return [tuple(t.float() for t in s) for s in R.sn_forward_sets(W.double(), u.double(), v.double(), 2)]


@pytest.mark.parametrize("form", ["plain", "accumulate", "second", "second+accumulate"])
@pytest.mark.parametrize("b", range(len(BATCHES)))
def test_spectral_norm_backward_meets_the_fp32_rule(ops, b, form):
    """dW = (G - <G, W_sn> u v^T) / sigma: plain; added to random prior contents (`accumulate_into`: the tensors handed in are the ones
    returned); with a second instance that has its own W_sn, u, v and sigma from a second power iteration.
    Largest e_k / e_t on the MI355X: dW 1.252."""
    batch = BATCHES[b]
    second, accumulate = "second" in form, "accumulate" in form
    args, args2, G, G2, prior = [[], [], [], [], []], [[], [], [], [], []], [], [], []
    for s in batch:
        c = R.sn_case(*key_of(s))
        i1, i2 = bwd_inputs(s[0], s[1])
        for k in range(4):
            args[k + 1].append(cu(i1[k]).reshape(-1)[:1].clone() if k == 3 else cu(i1[k]))
            args2[k + 1].append(cu(i2[k]).reshape(-1)[:1].clone() if k == 3 else cu(i2[k]))
        args[0].append(cu(c[3])); args2[0].append(cu(c[4])); prior.append(cu(c[5]).clone())
    got = ops.spectral_norm_bwd(*args, accumulate_into=prior if accumulate else None, second=tuple(args2) if second else None)
    for i, s in enumerate(batch):
        c = R.sn_case(*key_of(s))
        i1, i2 = bwd_inputs(s[0], s[1])
        if accumulate:
            assert got[i].data_ptr() == prior[i].data_ptr()
        res = []
        for cast in (torch.Tensor.double, torch.Tensor.float):
            res.append(R.sn_backward(cast(c[3]), *(cast(t) for t in i1), second=(cast(c[4]),) + tuple(cast(t) for t in i2) if second else None,
                                     accumulate_into=cast(c[5]) if accumulate else None))
        rule("dW %dx%d %s" % (s[0], s[1], form), got[i], res[0], res[1])


@pytest.mark.parametrize("rows, cols", [(5, 819), (257, 7)])
@pytest.mark.parametrize("flagged", [False, True])
def test_spectral_norm_backward_with_the_step_tail_is_bit_identical(ops, rows, cols, flagged):
    """`step=` (tp_sn_bwd_step: loss total + gate in kernel D, RMSprop in kernel E) at two ragged shapes against spectral_norm_bwd followed
    by weighted_sum(flags=) and rmsprop_step(gate=snapshot) -- what test_disc_step_tail_in_the_sn_backward_is_bit_identical compares at
    the PatchGAN's shapes: gradient, loss total, gate words, snapshot, parameters, square_avg and step counters, bit for bit; also on a
    flagged step (a NaN term), which must leave parameters and statistics as they are."""
    shapes = [(rows, cols), (3, 4)]
    state = []
    for fused in (True, False):
        rs = np.random.RandomState(rows)
        args, args2, params, sqs, steps = [[], [], [], [], []], [[], [], [], [], []], [], [], []
        for r, c_ in shapes:
            c = R.sn_case(r, c_)
            i1, i2 = bwd_inputs(r, c_)
            for k in range(4):
                args[k + 1].append(cu(i1[k]).reshape(-1)[:1].clone() if k == 3 else cu(i1[k]))
                args2[k + 1].append(cu(i2[k]).reshape(-1)[:1].clone() if k == 3 else cu(i2[k]))
            args[0].append(cu(c[3])); args2[0].append(cu(c[4]))
            params.append(cu(c[0]).clone())
            sqs.append(cu(torch.from_numpy(rs.uniform(0.0, 2.0, size=(r, c_)).astype(np.float32))))
            steps.append(torch.full((), 4.0, device=DEV))
        terms = [cu(torch.tensor(v, dtype=torch.float32)) for v in (0.7, float("nan") if flagged else 1.3, 0.25)]
        weights = [1.5, 10.0, 0.5]
        bad, snap = torch.zeros(4, dtype=torch.int32, device=DEV), torch.full((4,), 9, dtype=torch.int32, device=DEV)
        flags = dict(bad=bad, word_finite=2, snapshot=snap)
        lr = torch.tensor(3e-3, device=DEV)
        if fused:
            step = dict(terms=terms, weights=weights, flags=flags, params=params, square_avgs=sqs, steps=steps, lr=lr, alpha=0.99, eps=1e-8)
            grads = ops.spectral_norm_bwd(*args, second=tuple(args2), step=step)
            total = step["total"]
        else:
            grads = ops.spectral_norm_bwd(*args, second=tuple(args2))
            total = ops.weighted_sum(terms, weights, flags=flags)
            ops.rmsprop_step(params, grads, sqs, lr, alpha=0.99, eps=1e-8, gate=snap, steps=steps)
        state.append(grads + [total, bad, snap] + params + sqs + steps)
    assert len(state[0]) == len(state[1])
    for a, c in zip(*state):
        assert torch.equal(a, c) or (bool(torch.isnan(a).all()) and bool(torch.isnan(c).all()))
    bad, snap, p0, sq0, st0 = state[0][3], state[0][4], state[0][5], state[0][7], state[0][9]
    assert bad.tolist() == snap.tolist() == [0, 0, int(flagged), 0]
    assert float(st0) == (4.0 if flagged else 5.0)
    assert torch.equal(p0, cu(R.sn_case(rows, cols)[0])) == flagged


def test_spectral_norm_rejections_leave_the_library_usable(ops):
    """513 rows, 16385 columns, 9 weights, 0 and 4 sets: a TexposeLibraryError each (the set counts: from the C entry point; ops refuses
    them before it gets there), and a valid call afterwards still gives the right answer."""
    from texpose_amd import _lib

    def fresh(rows, cols, n=1):
        return ([torch.randn(rows, cols, device=DEV) for _ in range(n)], [torch.ones(rows, device=DEV) for _ in range(n)],
                [torch.ones(cols, device=DEV) for _ in range(n)])

    def valid_call_is_right():
        batch = ((5, 819), (3, 4))
        ws, us, vs = device_inputs(batch)
        outs, sig = ops.spectral_norm_fwd(ws, us, vs, True)
        for i, s in enumerate(batch):
            (r64, r32), = sn_ref(*key_of(s), "train")
            check_forward("%dx%d after a rejection" % s, (outs[i], us[i], vs[i], sig[i]), r64, r32)

    for rows, cols, n in ((513, 8, 1), (2, 16385, 1), (2, 3, 9)):
        with pytest.raises(_lib.TexposeLibraryError):
            ops.spectral_norm_fwd(*fresh(rows, cols, n), True)
        valid_call_is_right()
        if n == 1:
            with pytest.raises(_lib.TexposeLibraryError):
                ops.spectral_norm_fwd_sets(*fresh(rows, cols, n), 2)
            valid_call_is_right()
    with pytest.raises(_lib.TexposeLibraryError):
        g, ws_, u, v, sg = ([torch.ones(513, 8, device=DEV)], [torch.ones(513, 8, device=DEV)], [torch.ones(513, device=DEV)],
                            [torch.ones(8, device=DEV)], [torch.ones(1, device=DEV)])
        ops.spectral_norm_bwd(g, ws_, u, v, sg)
    valid_call_is_right()
    for n_sets in (0, 4):
        with pytest.raises(ValueError):
            ops.spectral_norm_fwd_sets(*fresh(5, 7), n_sets)
        # the entry point itself, with complete and distinct outputs for 4 sets of one weight: only the count is wrong
        (w,), (u,), (v,) = fresh(5, 7)
        arr = (_lib.SnWeight * 4)()
        wk = torch.empty(_lib.load().tp_sn_work_floats(5, 7), device=DEV)
        keep = [(torch.empty_like(w), torch.empty(1, device=DEV)) for _ in arr]
        for a, (o, sg) in zip(arr, keep):
            a.weight, a.u, a.v, a.weight_sn, a.sigma, a.work = w.data_ptr(), u.data_ptr(), v.data_ptr(), o.data_ptr(), sg.data_ptr(), wk.data_ptr()
            a.rows, a.cols = 5, 7
        with pytest.raises(_lib.TexposeLibraryError):
            _lib.check(_lib.load().tp_sn_fwd_sets(arr, 1, n_sets, torch.cuda.current_stream().cuda_stream), "tp_sn_fwd_sets")
        valid_call_is_right()


# ------------------------------------------------------------------------------------------ InstanceNorm2d + LeakyReLU
def nchw(t, n_inst, H, W):
    return cu(t).view(1, n_inst, H, W)


@functools.lru_cache(maxsize=None)
def inorm_bwd_refs(n_inst, H, W, values):
    """The backward kernels' inputs and what they must give: xhat and rstd are the REFERENCE's, rounded to float32 -- the gates every
    party takes from them are the fp64 xhat's (rounding keeps the sign), and kernel, fp64 restatement and fp32 evaluation start from the
    same numbers.  dict(xhat, rstd, r64 = (gx, gx + addend, g_gy, g_x), r32 = the same in fp32)."""
    c = R.inorm_case(n_inst, H, W, values)
    xhat, rstd = c["ref"]["xhat"].float(), c["ref"]["rstd"].float()
    assert torch.equal(xhat > 0, c["ref"]["xhat"] > 0)
    res = {}
    for name, cast in (("r64", torch.Tensor.double), ("r32", torch.Tensor.float)):
        xh, rs, gy, ggx, add = (cast(t) for t in (xhat, rstd, c["gy"], c["ggx"], c["addend"]))
        res[name] = (R.inorm_lrelu_bwd(xh, rs, gy, R.SLOPE), R.inorm_lrelu_bwd(xh, rs, gy, R.SLOPE, add)) + R.inorm_lrelu_bwd_bwd(xh, rs, gy, ggx, R.SLOPE)
    return dict(xhat=xhat, rstd=rstd, **res)


@pytest.mark.parametrize("values", R.INORM_VALUES)
@pytest.mark.parametrize("n_inst, H, W", R.INORM_SHAPES)
def test_inorm_lrelu_kernels_meet_the_fp32_rule(ops, n_inst, H, W, values):
    """Forward (y, xhat, rstd from x), backward (gx, with and without `addend`) and double backward (g_gy, g_x) at hw = 1, 2, 63, 64, 65,
    127, 4095, 4096 and 1, 3, 4, 5, 9 instances, for standard normal values, mean 1e3, spread 1e-3 and 1e3 (eps decides / vanishes) and
    one constant instance (xhat = y = 0 exactly, gate = slope everywhere).  gy and ggx are zero where |xhat_ref| < 1e-5 (norm_ref.inorm_case;
    at most 0.1 % of the elements, tests/test_norm_ref_cpu.py).
    Largest e_k / e_t on the MI355X over this module's tests: y 1.897, xhat 2.017, rstd 2.542, gx 1.270, g_gy 1.367, g_x 1.695."""
    c = R.inorm_case(n_inst, H, W, values)
    tag = "%dx%d (%dx%d) %s" % (n_inst, H * W, H, W, values)
    y, xhat, rstd = ops.inorm_lrelu_fwd(nchw(c["x"], n_inst, H, W), R.EPS, R.SLOPE)
    f32 = R.inorm_lrelu_fwd(c["x"], R.EPS, R.SLOPE)
    for name, got, want, t32 in (("y", y, c["ref"]["y"], f32[2]), ("xhat", xhat, c["ref"]["xhat"], f32[0]), ("rstd", rstd, c["ref"]["rstd"], f32[1])):
        rule("%s %s" % (name, tag), got.reshape(-1), want.reshape(-1), t32.reshape(-1))
    for r in torch.nonzero(c["exact"]).reshape(-1).tolist():
        assert not bool(xhat.view(n_inst, -1)[r].any()) and not bool(y.view(n_inst, -1)[r].any()), tag
    b = inorm_bwd_refs(n_inst, H, W, values)
    xh, rs = nchw(b["xhat"], n_inst, H, W), cu(b["rstd"])
    gy, ggx, addend = (nchw(c[k], n_inst, H, W) for k in ("gy", "ggx", "addend"))
    gx = ops.inorm_lrelu_bwd(xh, rs, gy, R.SLOPE)
    gx_add = ops.inorm_lrelu_bwd(xh, rs, gy, R.SLOPE, addend=addend)
    g_gy, g_x = ops.inorm_lrelu_bwd_bwd(xh, rs, gy, ggx, R.SLOPE)
    for name, got, want, t32 in zip(("gx", "gx +addend", "g_gy", "g_x"), (gx, gx_add, g_gy, g_x), b["r64"], b["r32"]):
        rule("%s %s" % (name, tag), got.reshape(-1), want.reshape(-1), t32.reshape(-1))
    if H * W == 1:
        assert not bool(gx.any()) and not bool(g_x.any()) and not bool(g_gy.any()), tag
        assert torch.equal(gx_add, addend)
    for r in torch.nonzero(c["exact"]).reshape(-1).tolist():                # gate = slope on the whole instance: an affine function of gy
        g = c["gy"][r].double()
        want = b["rstd"][r].double() * R.SLOPE * (g - g.mean())
        assert float((gx.view(n_inst, -1)[r].double().cpu() - want).abs().max()) <= 4 * float(np.spacing(np.float32(want.abs().max()))) * max(1, H * W) ** 0.5


@pytest.mark.parametrize("n_inst, H, W, values", [(5, 5, 13, "normal"), (3, 63, 65, "spread1e-3"), (9, 5, 13, "one_constant"), (5, 1, 1, "normal")])
def test_inorm_lrelu_autograd_is_the_chain_of_its_kernels(ops, n_inst, H, W, values):
    """autograd_ops.inorm_lrelu up to the second order hands each kernel the tensors the formulas name: its y, gx and the two second-order
    gradients are bit-identical to ops.inorm_lrelu_fwd -> _bwd -> _bwd_bwd on the forward's own xhat / rstd, and gx (which does not depend
    on a gate where gy is zero) is within the rule against the reference from x.
    Largest e_k / e_t of gx on the MI355X: 1.270 (over this module's tests)."""
    from texpose_amd import autograd_ops
    c = R.inorm_case(n_inst, H, W, values)
    x = nchw(c["x"], n_inst, H, W).clone().requires_grad_()
    gy = nchw(c["gy"], n_inst, H, W).clone().requires_grad_()
    u = nchw(c["ggx"], n_inst, H, W)
    y = autograd_ops.inorm_lrelu(x, R.EPS, R.SLOPE)
    (gx,) = torch.autograd.grad(y, x, gy, create_graph=True)
    g_x, g_gy = torch.autograd.grad((gx * u).sum(), (x, gy))
    y2, xhat, rstd = ops.inorm_lrelu_fwd(x.detach(), R.EPS, R.SLOPE)
    gx2 = ops.inorm_lrelu_bwd(xhat, rstd, gy.detach(), R.SLOPE)
    g_gy2, g_x2 = ops.inorm_lrelu_bwd_bwd(xhat, rstd, gy.detach(), u, R.SLOPE)
    for a, b_ in ((y, y2), (gx, gx2), (g_gy, g_gy2), (g_x, g_x2)):
        assert torch.equal(a.detach(), b_)
    t32 = R.inorm_lrelu(c["x"], R.EPS, R.SLOPE, c["gy"])["gx"]
    rule("gx chain %dx%d %s" % (n_inst, H * W, values), gx.detach().reshape(-1), c["ref"]["gx"].reshape(-1), t32.reshape(-1))


PAIRS = [((5, 5, 13), (3, 64, 64)), ((3, 63, 65), (9, 1, 1)), ((1, 1, 2), (4, 8, 8)), ((4, 7, 9), (5, 1, 127))]


@pytest.mark.parametrize("add_a, add_b", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("pa, pb", PAIRS)
def test_inorm_lrelu_backward_pair_is_bit_identical_to_single_launches(ops, pa, pb, add_a, add_b):
    """tp_inorm_lrelu_bwd_pair through ops.paired(): two problems of different (n_inst, hw) in one launch, `addend` on neither, either or
    both; first problems of 5, 3 and 1 instances leave the workgroup in front of the boundary `na` partly filled.  Each result equals its
    single launch bit for bit (and so meets the rule, test_inorm_lrelu_kernels_meet_the_fp32_rule)."""
    prob = []
    for (n_inst, H, W), add in ((pa, add_a), (pb, add_b)):
        c, b = R.inorm_case(n_inst, H, W, "normal"), inorm_bwd_refs(n_inst, H, W, "normal")
        prob.append((nchw(b["xhat"], n_inst, H, W), cu(b["rstd"]), nchw(c["gy"], n_inst, H, W), R.SLOPE, nchw(c["addend"], n_inst, H, W) if add else None))
    single = [ops.inorm_lrelu_bwd(*p) for p in prob]
    outs = [torch.full_like(p[0], float("nan")) for p in prob]
    with ops.paired():
        got = [ops.inorm_lrelu_bwd(*p, out=o) for p, o in zip(prob, outs)]
    for g, s, o in zip(got, single, outs):
        assert g.data_ptr() == o.data_ptr() and torch.equal(g, s)


def test_inorm_lrelu_forward_rejects_more_than_4096_elements(ops):
    """hw = 4097 does not fit the forward's registers: refused, and the next valid call is right."""
    from texpose_amd import _lib
    with pytest.raises(_lib.TexposeLibraryError):
        ops.inorm_lrelu_fwd(torch.randn(1, 2, 1, 4097, device=DEV), R.EPS, R.SLOPE)
    c = R.inorm_case(5, 5, 13, "normal")
    y, _, _ = ops.inorm_lrelu_fwd(nchw(c["x"], 5, 5, 13), R.EPS, R.SLOPE)
    rule("y after a rejection", y.reshape(-1), c["ref"]["y"].reshape(-1), R.inorm_lrelu_fwd(c["x"], R.EPS, R.SLOPE)[2].reshape(-1))


def test_inorm_lrelu_kernels_are_deterministic(ops):
    """Fixed-order wave reductions: each of the three kernels gives the same bits over 5 runs at (5, 4095)."""
    c, b = R.inorm_case(5, 63, 65, "normal"), inorm_bwd_refs(5, 63, 65, "normal")
    x, gy, ggx = (nchw(c[k], 5, 63, 65) for k in ("x", "gy", "ggx"))
    xh, rs = nchw(b["xhat"], 5, 63, 65), cu(b["rstd"])
    runs = []
    for _ in range(5):
        runs.append(ops.inorm_lrelu_fwd(x, R.EPS, R.SLOPE) + (ops.inorm_lrelu_bwd(xh, rs, gy, R.SLOPE),) + ops.inorm_lrelu_bwd_bwd(xh, rs, gy, ggx, R.SLOPE))
    for r in runs[1:]:
        assert len(r) == 6 and all(torch.equal(a, c_) for a, c_ in zip(r, runs[0]))
