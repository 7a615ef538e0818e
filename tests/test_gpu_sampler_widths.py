"""The sampler kernels at width edges against a float64 oracle, through the C ABI.

``tests/sampler_cases.py`` puts one small sampler on each boundary of
``samp_head_fwd`` / ``samp_head_bwd`` (every KPL, odd and short subtile
counts, one-row tiles, 33 tiles, padded categories, LDS pitches from Hm / D)
and on both fallbacks of the fused entry points (K > 1024, LDS > 160 KiB),
plus the plain Gaussian sampler at an odd B.  Each case runs
``abcd_sampler_forward_fused`` (with ``ppl_out``) and
``abcd_sampler_backward_split`` (both upstream gradients) in Gumbel mode with
the noise given and in softmax mode, and is compared with the oracle in
float64 on the un-padded model.

Tensors (logits, feats, d_h, every parameter gradient) are measured as
``test_gpu_edges.py`` measures them, in ``rel_err`` and ``block_err``, in units
of the fp32 oracle's own error ``e32``:

    e_hip <= R * e32 + 1e-7        and, whatever R,       e_hip <= 1e-4

with R = 4 unless ``R_TENSOR`` lists the (case, tensor); KL and the
perplexities keep ``LOSS_TOL`` = 1e-4 relative; ``argmax(logits)`` is exact on
every row (test_sampler_cases_cpu.py: every row's float64 top-2 gap is >= 1e-3).

Observed on MI355X (every figure is printed, ``-rA``; DESIGN.md s4,
profiles/parity_errors.json): worst e_hip 1.9e-6 (rel_err) and 3.4e-6
(block_err), both at k144_b33_tau01 (tau = 0.1, e32 3.5e-6 and 4.9e-6); KL
within 6e-7, the perplexities within 2e-6; only the two pairs of ``R_TENSOR``
are past R = 4.  Recorded without an R: feats with the Gumbel noise drawn
in-kernel, 4.5e-7 (rel_err) and 5.8e-7 (block_err).

Hygiene on every call: outputs are pre-filled with NaN, the workspace with
0xFF bytes before the forward (a stash the backward reads was written by the
forward), and every B-row output carries one guard row after row B - 1 that
must come back unchanged.  A padded case's padding must be exactly 0.
"""
import pytest
import torch

import sampler_cases as S
from edge_cases import dump_observed

pytestmark = pytest.mark.gpu

LOSS_TOL = 1e-4
HARD = 1e-4  # no tensor may exceed this in either metric, whatever R
R_DEFAULT = 4.0
# (case, tensor) -> R, raised only where that tensor exceeded 4 x e32 + 1e-7 on
# the GPU, to at most 2 x its own worst observed e_hip / e32 (in brackets), and
# only at the case where it did: everywhere else the tensor stays at 4.
R_NOTE = ("Neither is one of the fast intrinsics.  k16_b520, codebook gradient: dC = [d_feats; U]^T [Y; dL / sqrt(D)] "
          "is a single 16 x 16 tile there, summed over its 2 B = 1040 rows in one fp32 MFMA chain where torch's GEMM "
          "blocks the reduction; the fp32 operands summed row by row on the CPU give the GPU's error (1.1e-6; "
          "tests/test_sampler_cases_cpu.py::test_sequential_row_sum_moves_codebook_gradient).  k528_b1_peaked, "
          "posterior_shape_logits gradient: B = 1, so nothing averages and e32 (4.2e-8) is under one fp32 ulp; the "
          "kernel forms the prior gradient from an fp32 stash (p, alpha, trigamma(alpha): one rounding each) and Q "
          "through __expf (the fp32 oracle with exp2(x log2 e) in its softmax goes from 7e-8 to 1.2e-7); e_hip is "
          "2.8e-7, 4.6 ulp, against a bound of 2.7e-7 at R = 4 -- supposed, not separated further.")
_CB, _PSL = "g/feature_sampler/codebook", "g/feature_sampler/posterior_shape_logits"
R_TENSOR = {
    ("k16_b520", _CB): 9.0,         # [4.68, softmax: rel_err 1.12e-6 against 2.38e-7]
    ("k528_b1_peaked", _PSL): 13.0,  # [6.68, both modes: rel_err 2.77e-7 against 4.15e-8]
}
SENT = 12345.0  # the guard rows' sentinel
NAN = float("nan")


def ratio(case, key):
    return R_TENSOR.get((case, key), R_DEFAULT)


def _ck(rc):
    from modules import _native as N
    N.check(rc, "sampler widths test")


def _guarded(rows, width):
    """rows x width of NaN with one guard row of SENT after it; the view of the first rows."""
    buf = torch.full((rows + 1, width), NAN, device="cuda")
    buf[rows] = SENT
    return buf


def _guards_ok(out):
    for k, buf in out["guarded"].items():
        assert bool((buf[-1] == SENT).all()), f"{k}: the guard row after row B - 1 was written"


class Model:
    """A case's zero-padded twin on the device, its C-ABI structs and inputs."""

    def __init__(self, case):
        from modules import _native as N
        self.case, self.s = case, S.spec(case)
        s = self.s
        self.P = {k: v.cuda().contiguous() for k, v in S.padded_params(case).items()}
        c = N.SamplerCfg()
        c.input_size, c.mlp_hidden, c.feature_dim, c.plain = s.E, s.Hm, s.D, int(s.plain)
        c.num_categories = 16 if s.plain else s.K
        c.valid_categories = 0 if s.plain or s.Kv == s.K else s.Kv
        c.valid_feature_dim = 0 if s.Dv == s.D else s.Dv
        self.cfg = c
        self.mlps = [S._PPRE % k for k in range(2)] if s.plain else [S._PRE]
        p = N.SamplerParams()
        for k, pre in enumerate(self.mlps):
            for f, n in (("w1", ".0.weight"), ("b1", ".0.bias"), ("w2", ".2.weight"), ("b2", ".2.bias")):
                setattr(p.mlp[k], f, self.P[pre + n].data_ptr())
        if not s.plain:
            p.codebook, p.posterior_shape_logits = self.P[S.CB].data_ptr(), self.P[S.PSL].data_ptr()
            p.prior_concentration = s.a0
        self.par = p
        inp = S.inputs(case)
        pad = torch.nn.functional.pad
        self.h = inp["h"].cuda().contiguous()
        self.noise = pad(inp["noise"], (0, (s.D if s.plain else s.K) - inp["noise"].shape[1])).cuda().contiguous()
        self.d_feats = pad(inp["d_feats"], (0, s.D - s.Dv)).cuda().contiguous()
        self.d_kl = inp["d_kl"].clone().cuda()
        self.nbytes = N.lib().abcd_sampler_workspace_bytes(c, s.B)
        assert self.nbytes > 0
        self.width = 2 * s.D if s.plain else s.K  # of the logits / [mean | log_var]

    def grads(self):
        """NaN-filled gradient buffers of the padded shapes and their struct."""
        from modules import _native as N
        g = {k: torch.full_like(v, NAN) for k, v in self.P.items() if not k.endswith("prior_concentration")}
        st = N.SamplerGrads()
        for k, pre in enumerate(self.mlps):
            for f, n in (("w1", ".0.weight"), ("b1", ".0.bias"), ("w2", ".2.weight"), ("b2", ".2.bias")):
                setattr(st.mlp[k], f, g[pre + n].data_ptr())
        if not self.s.plain:
            st.codebook, st.posterior_shape_logits = g[S.CB].data_ptr(), g[S.PSL].data_ptr()
        return g, st

    def fresh_ws(self):
        from modules import _native as N
        ws = N.workspace(self.nbytes, "cuda")
        ws.fill_(0xFF)
        return ws

    def gmode(self, mode):
        from modules import _native as N
        return (N.SAMPLE_GUMBEL, self.s.tau) if mode == "gumbel" else (N.SAMPLE_SOFTMAX, 1.0)

    def forward(self, mode, ws, noise="given", seed=0, offset=0):
        from modules import _native as N
        s = self.s
        gm, tau = self.gmode(mode)
        logits, feats = _guarded(s.B, self.width), _guarded(s.B, s.D)
        kl = torch.tensor([NAN, SENT], device="cuda")
        ppl = torch.tensor([NAN, NAN, SENT], device="cuda")
        nz = self.noise if (noise == "given" and mode != "softmax") else None
        _ck(N.lib().abcd_sampler_forward_fused(self.cfg, self.par, N.ptr(self.h), s.B, gm, tau, N.ptr(nz), seed,
                                               offset, float(S.N_DATA), N.ptr(logits), N.ptr(feats), N.ptr(kl),
                                               None if s.plain else N.ptr(ppl), N.ptr(ws), ws.numel(), N.stream()))
        return dict(logits=logits[:s.B], feats=feats[:s.B], kl=kl, ppl=ppl,
                    guarded=dict(logits=logits, feats=feats, kl=kl[:, None], ppl=ppl[:, None]))

    def backward(self, mode, ws, out, d_feats=True, d_kl=True, wgrad=None):
        from modules import _native as N
        s = self.s
        gm, tau = self.gmode(mode)
        g, st = self.grads()
        d_h = _guarded(s.B, s.E)
        _ck(N.lib().abcd_sampler_backward_split(self.cfg, self.par, N.ptr(self.h), s.B, gm, tau, float(S.N_DATA),
                                                N.ptr(self.d_feats) if d_feats else None,
                                                N.ptr(self.d_kl) if d_kl else None, N.ptr(d_h), st, N.ptr(ws),
                                                ws.numel(), N.stream(), wgrad))
        out.update(d_h=d_h[:s.B], g=g, gst=st)
        out["guarded"]["d_h"] = d_h
        return out

    def run(self, mode, **kw):
        """Fused forward + one-call backward on a fresh 0xFF workspace; the dispatch names with it."""
        from modules import _native as N
        ws = self.fresh_ws()
        N.lib().abcd_dispatch_reset()
        out = self.backward(mode, ws, self.forward(mode, ws, **kw))
        torch.cuda.synchronize()
        out["ran"] = N.dispatch()
        _guards_ok(out)
        return out

    def valid(self, out, keys=None):
        """{tensor key: the real entries of the GPU's tensor}; every padding entry must be exactly 0."""
        s, hip = self.s, {}
        lg, ft = out["logits"], out["feats"]
        if s.plain:
            hip["logits"] = torch.cat([lg[:, :s.Dv], lg[:, s.D:s.D + s.Dv]], -1)
            rest = torch.cat([lg[:, s.Dv:s.D], lg[:, s.D + s.Dv:]], -1)
        else:
            hip["logits"], rest = lg[:, :s.Kv], lg[:, s.Kv:]
        assert not bool(rest.any()), "logits: padding columns are not exactly 0"
        hip["feats"] = ft[:, :s.Dv]
        assert not bool(ft[:, s.Dv:].any()), "feats: padding columns are not exactly 0"
        if "d_h" in out:
            hip["d_h"] = out["d_h"]
            for k, g in out["g"].items():
                val, rest = S.valid_slice(self.case, k, g)
                assert not bool(rest.any()), f"g/{k}: padding is not exactly 0"
                hip["g/" + k] = val
        return {k: v for k, v in hip.items() if keys is None or k in keys}


_MODELS = {}


def model(case):
    if case not in _MODELS:
        _MODELS[case] = Model(case)
    return _MODELS[case]


def _check_table(case, tag, hip, ref, record_property, fixed_R=True):
    """hip: {key: tensor}; ref: sampler_cases.reference().  Prints and records
    every figure, then asserts the bound and the hard 1e-4 on all of them
    (fixed_R False: the hard bound alone, the figures are recorded only)."""
    r64, e32 = ref["r64"], ref["e32"]
    rows, bad = [], []
    for k, t in hip.items():
        assert t.shape == r64[k].shape, (k, t.shape, r64[k].shape)
        assert bool(torch.isfinite(t).all()), f"{tag} {k}: NaN / Inf (an output or a stash that was never written)"
        if not r64[k].any():  # identically zero in exact arithmetic: the GPU must give exact zeros
            assert not bool(t.any()), (k, float(t.abs().max()))
            continue
        rel, blk = S.rel_err(t, r64[k]), S.block_err(t, r64[k])
        R = ratio(case, k) if fixed_R else None
        rows.append(dict(tensor=k, e32_rel=e32[k][0], e_hip_rel=rel, e32_blk=e32[k][1], e_hip_blk=blk, R=R))
        print(f"{tag} {k}: rel e32 {e32[k][0]:.2e} hip {rel:.2e} | blk e32 {e32[k][1]:.2e} hip {blk:.2e}")
        ok = rel <= HARD and blk <= HARD
        if fixed_R:
            ok = ok and rel <= R * e32[k][0] + 1e-7 and blk <= R * e32[k][1] + 1e-7
        if not ok:
            bad.append((k, rel, e32[k][0], blk, e32[k][1]))
    record_property("parity_errors", rows)
    dump_observed(tag, rows)
    assert not bad, bad


def _check_scalars(tag, out, r64, plain):
    kl = float(out["kl"][0])
    print(f"{tag} kl: hip {kl:.9g} ref {r64['kl']:.9g} rel {abs(kl - r64['kl']) / abs(r64['kl']):.2e}")
    assert abs(kl - r64["kl"]) <= LOSS_TOL * abs(r64["kl"]), (kl, r64["kl"])
    if plain:
        return
    for i, name in enumerate(("cluster_ppl", "batch_ppl")):
        v, r = float(out["ppl"][i]), r64["ppl"][i]
        print(f"{tag} {name}: hip {v:.9g} ref {r:.9g} rel {abs(v - r) / abs(r):.2e}")
        assert abs(v - r) <= LOSS_TOL * abs(r), (name, v, r)


def _check_dispatch(case, ran):
    head_fwd = "samp_head_fwd grid %d" % S.tiles(S.spec(case).B) in ran["samp_fwd"][0]
    head_bwd = ran["samp_bwd"][0].startswith("samp_head_bwd")
    assert head_fwd == head_bwd == S.fused(case), (case, ran["samp_fwd"], ran["samp_bwd"])
    assert S.fused(case) == (case not in S.FALLBACK)


@pytest.mark.parametrize("mode", S.MODES)
@pytest.mark.parametrize("case", S.ABCD_CASES)
def test_sampler_widths_vs_oracle64(case, mode, record_property):
    m, ref = model(case), S.reference(case, mode)
    out = m.run(mode)
    _check_dispatch(case, out["ran"])
    hip = m.valid(out)
    assert set(hip) == set(S.tensor_keys(case))
    tag = f"samp-{case}-{mode}"
    _check_scalars(tag, out, ref["r64"], False)
    assert float(S.top2_gaps(ref["r64"]["logits"]).min()) >= S.ARGMAX_GAP
    assert torch.equal(hip["logits"].argmax(-1).cpu(), ref["r64"]["logits"].argmax(-1))
    _check_table(case, tag, hip, ref, record_property)


def test_plain_sampler_vs_oracle64(record_property):
    case = "plain_b17"
    m, ref = model(case), S.reference(case, "plain")
    out = m.run("plain")
    assert "samp_head" not in out["ran"]["samp_fwd"][0] + out["ran"]["samp_bwd"][0]
    hip = m.valid(out)
    assert set(hip) == set(S.tensor_keys(case))
    _check_scalars("samp-" + case, out, ref["r64"], True)
    _check_table(case, "samp-" + case, hip, ref, record_property)


@pytest.mark.parametrize("term", ["feats", "kl", "none"])
def test_backward_branches_single_term(term, record_property):
    """d_kl = NULL / d_feats = NULL (the per-method pieces inside
    abcd_sampler_backward_split) against the float64 gradient of that term
    alone; posterior_shape_logits' gradient without d_kl, and everything
    without either, is exactly 0 (the memsets)."""
    case = "k80_b17"
    m = model(case)
    ws = m.fresh_ws()
    out = m.backward("gumbel", ws, m.forward("gumbel", ws), d_feats=term == "feats", d_kl=term == "kl")
    torch.cuda.synchronize()
    _guards_ok(out)
    hip = m.valid(out, keys=S.tensor_keys(case)[2:])
    if term == "none":
        for k, t in hip.items():
            assert bool(torch.isfinite(t).all()) and not bool(t.any()), (k, float(t.abs().max()))
        return
    ref = S.reference(case, "gumbel", term)
    if term == "feats":
        assert not ref["r64"]["g/" + S.PSL].any() and not bool(hip["g/" + S.PSL].any())
    _check_table(case, f"samp-{case}-d_{term}_only", hip, ref, record_property)


def test_deferred_parameter_gradients_off_bench_widths():
    """ABCD_DEFER_PARAMS then abcd_sampler_backward_params at K = 144 (KPL 4,
    three tiles): the same bits as the one-call backward."""
    from modules import _native as N
    case = "k144_b33_tau01"
    m, s = model(case), S.spec(case)
    assert S.fused(case)
    one = m.run("gumbel")
    ws = m.fresh_ws()
    two = m.backward("gumbel", ws, m.forward("gumbel", ws), wgrad=N.DEFER_PARAMS)
    torch.cuda.synchronize()
    for k in (S.CB, S._PRE + ".0.weight", S._PRE + ".2.weight"):
        assert bool(torch.isnan(two["g"][k]).all()), f"{k}: written before abcd_sampler_backward_params"
    _ck(N.lib().abcd_sampler_backward_params(m.cfg, m.par, N.ptr(m.h), s.B, two["gst"], N.ptr(ws), ws.numel(),
                                             N.stream(), None))
    torch.cuda.synchronize()
    _guards_ok(two)
    assert torch.equal(one["d_h"], two["d_h"])
    for k in one["g"]:
        assert bool(torch.isfinite(two["g"][k]).all()), k
        assert torch.equal(one["g"][k], two["g"][k]), (k, float((one["g"][k] - two["g"][k]).abs().max()))


@pytest.mark.parametrize("mode", S.MODES)
def test_per_method_path_vs_oracle64(mode, record_property):
    """abcd_sampler_forward / _sample / _kl and their three backward pieces at
    K = 272 (260 valid): the same bounds against the float64 oracle as the
    fused path, so both are pinned to the reference and not only to each other."""
    from modules import _native as N
    L = N.lib()
    case = "k272pad_b15"
    m, s, ref = model(case), S.spec(case), S.reference(case, mode)
    gm, tau = m.gmode(mode)
    st = N.stream()
    ws = m.fresh_ws()
    logits, feats = _guarded(s.B, s.K), _guarded(s.B, s.D)
    kl = torch.tensor([NAN, SENT], device="cuda")
    nz = m.noise if mode == "gumbel" else None
    _ck(L.abcd_sampler_forward(m.cfg, m.par, N.ptr(m.h), s.B, N.ptr(logits), N.ptr(ws), ws.numel(), st))
    _ck(L.abcd_sampler_sample(m.cfg, m.par, N.ptr(logits), s.B, gm, tau, N.ptr(nz), 0, 0, N.ptr(feats), N.ptr(ws),
                              ws.numel(), st))
    _ck(L.abcd_sampler_kl(m.cfg, m.par, N.ptr(logits), s.B, float(S.N_DATA), N.ptr(kl), N.ptr(ws), ws.numel(), st))
    g, gst = m.grads()
    dl, d_h = _guarded(s.B, s.K), _guarded(s.B, s.E)
    _ck(L.abcd_sampler_sample_backward(m.cfg, m.par, s.B, gm, tau, N.ptr(m.d_feats), N.ptr(dl), N.ptr(g[S.CB]),
                                       N.ptr(ws), ws.numel(), st))
    _ck(L.abcd_sampler_kl_backward(m.cfg, m.par, s.B, float(S.N_DATA), N.ptr(m.d_kl), 1, N.ptr(dl),
                                   N.ptr(g[S.PSL]), N.ptr(ws), ws.numel(), st))
    _ck(L.abcd_sampler_forward_backward(m.cfg, m.par, N.ptr(m.h), s.B, N.ptr(dl), N.ptr(d_h), gst, 1, N.ptr(ws),
                                        ws.numel(), st))
    torch.cuda.synchronize()
    out = dict(logits=logits[:s.B], feats=feats[:s.B], kl=kl, d_h=d_h[:s.B], g=g,
               guarded=dict(logits=logits, feats=feats, kl=kl[:, None], dl=dl, d_h=d_h))
    _guards_ok(out)
    hip = m.valid(out)
    tag = f"samp-{case}-{mode}-per_method"
    kv = float(kl[0])
    print(f"{tag} kl: hip {kv:.9g} ref {ref['r64']['kl']:.9g}")
    assert abs(kv - ref["r64"]["kl"]) <= LOSS_TOL * abs(ref["r64"]["kl"])
    assert torch.equal(hip["logits"].argmax(-1).cpu(), ref["r64"]["logits"].argmax(-1))
    _check_table(case, tag, hip, ref, record_property)


def test_in_kernel_gumbel_crosses_the_counter_carry(record_property):
    """noise = NULL: the head draws Gumbel noise from Philox(seed, offset + b K
    + k).  With offset = 2^32 - 7 K row 7 starts exactly at the counter's carry
    into its high word.  Against the float64 oracle fed with the numpy stream:
    logits bit-equal to the given-noise run, feats under the hard 1e-4 (the
    device's fast log on the noise is the unknown: the figure is recorded, no R
    is fixed in advance)."""
    case = "k80_b17"
    m, s = model(case), S.spec(case)
    seed, offset = 1234, 2 ** 32 - 7 * s.K
    idx = S.indices(offset, s.B * s.K)
    assert int(idx[7 * s.K]) == 2 ** 32 and int(idx[7 * s.K - 1]) == 2 ** 32 - 1
    g = torch.from_numpy(S.gumbel(seed, idx).reshape(s.B, s.K))
    r64 = S.run_oracle(case, "gumbel", torch.float64, noise=g)
    r32 = S.run_oracle(case, "gumbel", torch.float32, noise=g)
    ref = dict(r64=r64, e32={k: (S.rel_err(r32[k], r64[k]), S.block_err(r32[k], r64[k])) for k in ("logits", "feats")})
    given = m.run("gumbel")
    out = m.run("gumbel", noise=None, seed=seed, offset=offset)
    assert S.fused(case) and "samp_head_fwd" in out["ran"]["samp_fwd"][0]
    assert torch.equal(out["logits"], given["logits"])
    assert not torch.equal(out["feats"], given["feats"])
    hip = m.valid(out, keys=("feats",))
    # a stream that ignored the carry (row 7 on restarting at index 0) or the high word is O(1) off
    wrong = torch.from_numpy(S.gumbel(seed, idx & S._M32).reshape(s.B, s.K))
    assert S.rel_err(S.run_oracle(case, "gumbel", torch.float64, noise=wrong)["feats"], r64["feats"]) > 1e-2
    _check_table(case, f"samp-{case}-gumbel_philox", hip, ref, record_property, fixed_R=False)
    # the per-method sample kernel draws the same stream
    from modules import _native as N
    ws = m.fresh_ws()
    fwd = m.forward("gumbel", ws)
    feats = _guarded(s.B, s.D)
    _ck(N.lib().abcd_sampler_sample(m.cfg, m.par, N.ptr(fwd["logits"]), s.B, N.SAMPLE_GUMBEL, s.tau, None, seed,
                                    offset, N.ptr(feats), N.ptr(ws), ws.numel(), N.stream()))
    torch.cuda.synchronize()
    assert bool((feats[-1] == SENT).all())
    assert S.rel_err(feats[:s.B, :s.Dv], r64["feats"]) <= HARD and S.block_err(feats[:s.B, :s.Dv], r64["feats"]) <= HARD
