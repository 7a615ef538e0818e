"""abcd_grad_norm, abcd_clip_sgd and abcd_total_loss (abcd_optim.hip) against
float64, through the C ABI.

``sq_norm`` reads the gradient as float4 with a scalar ``n % 4`` tail over a
fixed 256 x 256 grid, accumulates in fp64 and hands the partials to its last
workgroup through a self-resetting ticket; ``sgd_update`` is a grid-stride
pass of at most 4096 x 256 threads.  The sizes sit on those edges: n below 4,
on and around it, around one block, and 65537 / 262147 / 1048579 (one past the
sq_norm grid's thread count, past its float4 reach, past one sgd_update pass;
n % 4 = 1, 3, 3).

Reference, in float64 on the fp32 inputs: norm = sqrt(sum g^2),
coef = min(max_norm / (norm + 1e-6), 1).  Bounds, from the arithmetic:

* the norm: 1 ulp of fp32 (an fp64 sum, one rounding at the cast);
* the clipped gradient: 2^-21 relative -- four fp32 roundings (norm, add,
  divide, multiply) at 2^-24 each, doubled;
* the parameter: 2^-24 |p_ref| for its own rounding plus 2^-21 |lr b_ref| for
  the step's, b_ref = coef g, or m buf + coef g with momentum;
* the momentum buffer: 2^-21 (|m buf| + |coef g|).

The parameter bound is relative to |lr b_ref|, which fp32 can meet only where
m buf + coef g does not cancel: the second momentum step's gradient takes the
buffer's signs.

Buffers are torch allocations passed at their base; outputs are pre-filled
with NaN, the workspace with 0xFF bytes, and each array has four guard
elements after element n - 1 that must come back unchanged.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 4, 5, 255, 257, 65537, 262147, 1048579]
SENT = 12345.0
GUARD = 4
NAN = float("nan")
E21, E24 = 2.0 ** -21, 2.0 ** -24


def _lib():
    from modules import _native as N
    return N, N.lib()


def _ws(n, fill=0xFF):
    N, L = _lib()
    ws = N.workspace(L.abcd_optim_workspace_bytes(n), "cuda")
    ws.fill_(fill)
    return ws


def _dev(x):
    """x (CPU fp32, n values) on the device with GUARD sentinel elements after it."""
    buf = torch.full((x.numel() + GUARD,), SENT, device="cuda")
    buf[:x.numel()] = x.cuda()
    return buf


def _guard_ok(buf, n):
    assert bool((buf[n:] == SENT).all()), "written past element n - 1"


def _ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


def _f32(x):
    """x rounded to fp32 (what the C ABI's float arguments receive), as a Python float."""
    return float(np.float32(x))


def _randn(n, seed, scale=1.0):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed)) * scale


def _ref(g, max_norm):
    norm = float(g.double().pow(2).sum().sqrt())
    return norm, min(max_norm / (norm + 1e-6), 1.0)


def _grad_norm(g):
    N, L = _lib()
    n = g.numel()
    gd, out, ws = _dev(g), torch.tensor([NAN, SENT], device="cuda"), _ws(n)
    N.check(L.abcd_grad_norm(N.ptr(gd), n, N.ptr(out), N.ptr(ws), ws.numel(), N.stream()), "abcd_grad_norm")
    torch.cuda.synchronize()
    assert float(out[1]) == SENT
    assert torch.equal(gd[:n].cpu(), g), "abcd_grad_norm changed the gradient"
    _guard_ok(gd, n)
    return float(out[0])


@pytest.mark.parametrize("n", SIZES)
def test_grad_norm(n):
    g = _randn(n, 100 + n, 0.37)
    norm, ref = _grad_norm(g), _ref(g, 1.0)[0]
    print(f"n {n}: norm {norm:.9g} ref {ref:.9g} ulps {abs(norm - ref) / _ulp32(ref):.3f}")
    assert abs(norm - ref) <= _ulp32(ref), (norm, ref)


@pytest.mark.parametrize("n", [1, 5, 65537, 1048579])
def test_grad_norm_accumulates_in_fp64(n):
    """Gradients of magnitude 1e20: their squares overflow fp32, the norm does not."""
    g = _randn(n, 200 + n, 1e20)
    assert not torch.isfinite(g.pow(2).sum())  # what an fp32 accumulation gives
    norm, ref = _grad_norm(g), _ref(g, 1.0)[0]
    assert np.isfinite(norm) and abs(norm - ref) <= _ulp32(ref), (norm, ref)
    # and tiny ones, whose squares underflow fp32
    g = _randn(n, 300 + n, 1e-25)
    norm, ref = _grad_norm(g), _ref(g, 1.0)[0]
    assert norm > 0 and abs(norm - ref) <= _ulp32(ref), (norm, ref)


def _clip_sgd(p, g, buf, max_norm, lr, momentum, init, ws=None, want_norm=True, sync=True):
    """One abcd_clip_sgd on guarded device buffers (_dev), in place; returns the norm slot."""
    N, L = _lib()
    n = g.numel() - GUARD
    out = torch.tensor([NAN, SENT], device="cuda")
    ws = _ws(n) if ws is None else ws
    N.check(L.abcd_clip_sgd(N.ptr(p), N.ptr(g), N.ptr(buf), n, max_norm, lr, momentum, init,
                            N.ptr(out) if want_norm else None, N.ptr(ws), ws.numel(), N.stream()), "abcd_clip_sgd")
    if sync:
        torch.cuda.synchronize()
    return out


def _check_step(tag, p0, g0, buf0, pd, gd, bufd, out, max_norm, lr, momentum, init):
    """The device's p / g / buf after one step against the float64 step from (p0, g0, buf0)."""
    n = g0.numel()
    norm, coef = _ref(g0, max_norm)
    for b in (pd, gd) + ((bufd,) if bufd is not None else ()):
        _guard_ok(b, n)
    if out is not None:
        assert float(out[1]) == SENT
        assert abs(float(out[0]) - norm) <= _ulp32(norm), (float(out[0]), norm)
    cg = coef * g0.double()
    g_out = gd[:n].cpu().double()
    eg = ((g_out - cg).abs() - E21 * cg.abs()).max().item()
    assert eg <= 0, (tag, "g", eg)
    if coef == 1.0:
        assert torch.equal(gd[:n].cpu(), g0), (tag, "un-clipped: the gradient must come back bit-equal")
    b_ref, b_mag = cg, cg.abs()
    if momentum != 0.0:
        if not init:
            mb = momentum * buf0.double()
            b_ref, b_mag = mb + cg, mb.abs() + cg.abs()
        eb = ((bufd[:n].cpu().double() - b_ref).abs() - E21 * b_mag).max().item()
        assert eb <= 0, (tag, "momentum buffer", eb)
    p_ref = p0.double() - lr * b_ref
    ep = ((pd[:n].cpu().double() - p_ref).abs() - E24 * p_ref.abs() - E21 * (lr * b_ref).abs()).max().item()
    assert ep <= 0, (tag, "p", ep)
    worst_g = ((g_out - cg).abs() / cg.abs().clamp_min(1e-300)).max().item() if cg.any() else 0.0
    print(f"{tag} n {n}: norm {norm:.6g} coef {coef:.6g} worst g rel {worst_g / E24:.2f} x 2^-24")
    return norm, coef


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", ["clipped", "unclipped", "zero"])
def test_clip_sgd_momentum_0(n, kind):
    """momentum 0 with momentum_buf = NULL."""
    p0 = _randn(n, 400 + n)
    g0 = torch.zeros(n) if kind == "zero" else _randn(n, 500 + n, 0.37)
    norm = _ref(g0, 1.0)[0]
    max_norm = _f32({"clipped": norm / 30.0, "unclipped": 2.0 * norm + 1e-3, "zero": 1.0}[kind])
    lr = _f32(0.7)
    pd, gd = _dev(p0), _dev(g0)
    out = _clip_sgd(pd, gd, None, max_norm, lr, 0.0, 0)
    norm, coef = _check_step(kind, p0, g0, None, pd, gd, None, out, max_norm, lr, 0.0, 0)
    if kind == "clipped":
        assert 0.03 < coef < 0.034
    if kind == "unclipped":
        assert coef == 1.0
    if kind == "zero":  # norm 0, nothing moves
        assert float(out[0]) == 0.0 and torch.equal(pd[:n].cpu(), p0) and not bool(gd[:n].any())


@pytest.mark.parametrize("n", SIZES)
def test_clip_sgd_momentum(n):
    """momentum 0.9: momentum_init = 1 (the buffer, holding NaN, is overwritten
    with the clipped gradient), then momentum_init = 0 on a second gradient;
    the second call has out_norm = NULL."""
    lr, mom = 0.5, _f32(0.9)
    p0, g0 = _randn(n, 600 + n), _randn(n, 700 + n, 0.37)
    max_norm = _f32(_ref(g0, 1.0)[0] / 30.0)
    pd, gd = _dev(p0), _dev(g0)
    bufd = _dev(torch.full((n,), NAN))
    out = _clip_sgd(pd, gd, bufd, max_norm, lr, mom, 1)
    _check_step("init", p0, g0, None, pd, gd, bufd, out, max_norm, lr, mom, 1)
    p1, buf1 = pd[:n].cpu(), bufd[:n].cpu()
    assert bool(torch.isfinite(buf1).all())
    sign = torch.where(buf1 < 0, -1.0, 1.0)
    g1 = _randn(n, 800 + n, 0.21).abs() * sign  # no cancellation in m buf + coef g (see the module docstring)
    gd = _dev(g1)
    max_norm = _f32(0.8 * _ref(g1, 1.0)[0])
    _clip_sgd(pd, gd, bufd, max_norm, lr, mom, 0, want_norm=False)
    _check_step("step2", p1, g1, buf1, pd, gd, bufd, None, max_norm, lr, mom, 0)


def test_ticket_resets_between_back_to_back_calls():
    """Three abcd_clip_sgd calls (n = 5, 1048579, 257) on one stream into one
    workspace with no synchronise between them: each gets its own norm (the
    last workgroup's ticket resets itself, the partials of one call are not
    read by the next), and a second identical run gives the same bits."""
    sizes = [5, 1048579, 257]
    N, L = _lib()
    runs = []
    for _ in range(2):
        ws = _ws(max(sizes))
        state = []
        for n in sizes:
            p0, g0 = _randn(n, 900 + n), _randn(n, 1000 + n, 0.37 * (1 + n % 7))
            state.append((p0, g0, _dev(p0), _dev(g0)))
        outs = [_clip_sgd(pd, gd, None, 1.0, 1.0, 0.0, 0, ws=ws, sync=False) for _, _, pd, gd in state]
        torch.cuda.synchronize()
        for (p0, g0, pd, gd), out in zip(state, outs):
            _check_step("ticket", p0, g0, None, pd, gd, None, out, 1.0, 1.0, 0.0, 0)
        norms = [float(o[0]) for o in outs]
        assert len(set(norms)) == 3, norms
        runs.append([t.clone() for _, _, pd, gd in state for t in (pd, gd)] + outs)
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_argument_errors():
    """Refused before any launch: ABCD_EINVAL, nothing written."""
    N, L = _lib()
    n = 8
    p, g, buf = _dev(_randn(n, 1)), _dev(_randn(n, 2)), _dev(torch.zeros(n))
    keep = [t.clone() for t in (p, g, buf)]
    out = torch.tensor([NAN, SENT], device="cuda")
    ws = _ws(n)
    nbytes = L.abcd_optim_workspace_bytes(n)
    assert 0 < nbytes <= ws.numel()
    st = N.stream()
    calls = [
        L.abcd_clip_sgd(N.ptr(p), N.ptr(g), None, 0, 1.0, 1.0, 0.0, 0, N.ptr(out), N.ptr(ws), nbytes, st),
        L.abcd_clip_sgd(N.ptr(p), N.ptr(g), None, n, 1.0, 1.0, 0.0, 0, N.ptr(out), N.ptr(ws), nbytes - 1, st),
        L.abcd_clip_sgd(N.ptr(p), N.ptr(g), None, n, 1.0, 1.0, 0.9, 1, N.ptr(out), N.ptr(ws), nbytes, st),
        L.abcd_grad_norm(N.ptr(g), 0, N.ptr(out), N.ptr(ws), nbytes, st),
        L.abcd_grad_norm(N.ptr(g), n, N.ptr(out), N.ptr(ws), nbytes - 1, st),
    ]
    torch.cuda.synchronize()
    assert calls == [N.ABCD_EINVAL] * len(calls), calls
    for a, b in zip((p, g, buf), keep):
        assert torch.equal(a, b)
    assert bool(torch.isnan(out[0])) and float(out[1]) == SENT
    assert bool((ws == 0xFF).all())


@pytest.mark.parametrize("B", [1, 513])
def test_total_loss(B):
    N, L = _lib()
    g = torch.Generator().manual_seed(B)
    losses = torch.rand(2, generator=g) * 1e4 + 1.0
    kl = torch.rand(1, generator=g) * 50 + 0.1
    ld, kd = _dev(losses), _dev(kl)
    out = torch.tensor([NAN, SENT], device="cuda")
    N.check(L.abcd_total_loss(N.ptr(ld), N.ptr(kd), B, N.ptr(out), N.stream()), "abcd_total_loss")
    torch.cuda.synchronize()
    ref = float((losses.double().sum() + kl.double()[0]) / B)
    print(f"B {B}: loss {float(out[0]):.9g} ref {ref:.9g} ulps {abs(float(out[0]) - ref) / _ulp32(ref):.3f}")
    assert abs(float(out[0]) - ref) <= 2 * _ulp32(ref), (float(out[0]), ref)
    assert float(out[1]) == SENT
    _guard_ok(ld, 2)
    _guard_ok(kd, 1)
    assert L.abcd_total_loss(N.ptr(ld), N.ptr(kd), 0, N.ptr(out), N.stream()) == N.ABCD_EINVAL
