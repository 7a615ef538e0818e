"""Free-running generation (``abcd_decoder_generate``,
``RNN_Variational_Decoder.generate``, ``decode.py``) against the float64
reference of ``gen_cases.py``: the oracle decoder on the full rectangle, then
the stop rule, the stable sort and the repacking in numpy.

Lengths, order, batch_sizes and total are compared exactly (every stop decision
of the reference clears ``gen_cases.STOP_GAP``, see test_generate_cpu.py); the
packed tensors by ``edge_cases.rel_err`` (max |a - ref| / max |ref|) under the
1e-4 bar of test_gpu_edges.py.  Every figure is printed (``-rA``).
"""
import os

import numpy as np
import pytest
import torch

import edge_cases as E
import gen_cases as G
from gpu_helpers import build_from_meta, named_params

pytestmark = pytest.mark.gpu

HARD = 1e-4
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _bench_modules(ref):
    """enc, samp, dec at a bench.py width set, seed-1111 weights (checked against the oracle's)."""
    from modules import model as M
    cfg = ref["meta"]
    torch.manual_seed(1111)
    enc = M.RNN_Variational_Encoder(cfg["F"], cfg["H"], rnn_type=cfg["rnn"])
    samp = M.ABCDSampler(enc.hidden_size_total, cfg["Hm"], cfg["K"], cfg["D"])
    dec = M.RNN_Variational_Decoder(cfg["F"], cfg["H"], cfg["Hm"], cfg["D"], rnn_type=cfg["rnn"],
                                    num_speakers=cfg["spk"] or None, speaker_embed_dim=cfg["sdim"])
    for m in (enc, samp, dec):
        m.cuda().eval()
    for k, p in named_params(enc, samp, dec).items():
        assert torch.equal(p.detach().cpu(), ref["P"][k]), k
    return enc, samp, dec


def _odd_modules(ref):
    enc, samp, dec = build_from_meta(ref["meta"], load_arr(), device="cuda")
    for m in (enc, samp, dec):
        m.eval()
    return enc, samp, dec


def load_arr():
    from golden_io import load_small
    return load_small("lstm_odd")[1]


def abi_generate(cfg_list, params, feats, spk, B, T, mode, eps, seed, offset, stop_logit, min_len):
    """abcd_decoder_generate through ctypes -> (rc, outputs on the host)."""
    from modules import _native as N, ops
    L_ = N.lib()
    c = ops._dec_cfg(cfg_list)
    F = int(cfg_list[0])
    rows = max(B * T, 1)
    ws = N.workspace(L_.abcd_decoder_generate_workspace_bytes(c, T, B), "cuda")
    out, mu, lv = (torch.full((rows, F), float("nan"), device="cuda") for _ in range(3))
    offl = torch.full((rows,), float("nan"), device="cuda")
    lengths = torch.full((max(B, 1),), -1, dtype=torch.int32, device="cuda")
    order = torch.full((max(B, 1),), -1, dtype=torch.int64, device="cuda")
    bs = torch.full((max(T, 1),), -1, dtype=torch.int64, device="cuda")
    total = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    rc = L_.abcd_decoder_generate(c, ops._dec_struct(cfg_list, params), N.ptr(feats), N.ptr(spk), B, T, mode,
                                  N.ptr(eps), seed, offset, stop_logit, min_len, N.ptr(out), N.ptr(mu), N.ptr(lv),
                                  N.ptr(offl), N.ptr(lengths), N.ptr(order), N.ptr(bs), N.ptr(total), N.ptr(ws),
                                  ws.numel(), N.stream())
    torch.cuda.synchronize()
    return rc, dict(out=out.cpu(), mu=mu.cpu(), lv=lv.cpu(), logits=offl.cpu(), lengths=lengths.cpu().numpy(),
                    order=order.cpu().numpy(), batch_sizes=bs.cpu().numpy(), total=int(total.cpu()))


def check_against(tag, got, ref):
    """got: lengths / order / batch_sizes / total and packed out / mu / lv / logits (>= total rows)."""
    assert got["lengths"].tolist() == ref["lengths"].tolist()
    assert got["order"].tolist() == ref["order"].tolist()
    assert got["batch_sizes"].tolist() == ref["batch_sizes"].tolist()
    assert got["total"] == ref["total"]
    n = ref["total"]
    for k in ("out", "mu", "lv", "logits"):
        a = got[k][:n]
        assert torch.isfinite(a).all(), k
        e = E.rel_err(a, ref["packed"][k])
        print(f"{tag} {k}: rel_err {e:.2e} (rows {n})")
        assert e < HARD, (k, e)


@pytest.mark.parametrize("name", ["c2_mean", "c2gru_sample", "c5gru_mean"])
def test_generate_abi_vs_oracle64(name):
    from modules import _native as N
    ref = G.reference(name)
    c = ref["case"]
    _, _, dec = _bench_modules(ref)
    spk = ref["speakers"].cuda() if ref["ocfg"]["num_speakers"] else None
    eps = ref["eps"].cuda() if c["mode"] == G.SAMPLE else None
    N.lib().abcd_dispatch_reset()
    rc, got = abi_generate(dec._cfg_list(1), dec._param_list(), ref["feats"].cuda(), spk, c["B"], c["T"], c["mode"],
                           eps, 0, 0, ref["stop_logit"], c["min_len"])
    assert rc == 0
    assert N.lib().abcd_device_status() == 0
    kern, count = N.dispatch()["dec_fwd"]
    print(name, "dec_fwd:", kern)
    # the persistent form, once: no per-step fallback
    assert kern.startswith("dec_fwd_x6<") and ref["meta"]["rnn"] in kern and count == 1, (kern, count)
    check_against(name, got, ref)
    if c["mode"] == G.MEAN:  # eps = 0: the emitted frame is the mean itself
        n = ref["total"]
        assert torch.equal(got["out"][:n].view(torch.int32), got["mu"][:n].view(torch.int32))
    else:
        assert not torch.equal(got["out"][:ref["total"]], got["mu"][:ref["total"]])


@pytest.mark.parametrize("persist", ["1", "0"])
def test_generate_module_odd_feeds_encoder(persist, monkeypatch):
    """Sizes off the 16-grid through decoder.generate() (stop_prob, the padded
    twin), and its PackedSequence straight into the encoder.  At the twin's
    H = 32 the forward is the older persistent form (dec_fwd_persist); with
    ABCD_PERSIST=0 it is the per-step kernels."""
    from modules import _native as N
    from oracle import abcd_oracle as O
    ref = G.reference("odd_mean")
    c = ref["case"]
    enc, _, dec = _odd_modules(ref)
    monkeypatch.setenv("ABCD_PERSIST", persist)
    N.lib().abcd_dispatch_reset()
    packed, lengths, (mu, lv), offl = dec.generate(ref["feats"].cuda(), c["T"], speaker=ref["speakers"].cuda(),
                                                   mean=True, stop_prob=c["stop_prob"], min_length=c["min_len"])
    torch.cuda.synchronize()
    kern, count = N.dispatch()["dec_fwd"]
    print("odd dec_fwd:", kern)
    assert kern.startswith("dec_fwd_persist" if persist == "1" else "per-step decoder forward") and count == 1, kern
    assert isinstance(packed, torch.nn.utils.rnn.PackedSequence)
    assert packed.batch_sizes.device.type == "cpu" and packed.batch_sizes.dtype == torch.int64
    nz = [int(b) for b in ref["batch_sizes"] if b > 0]
    assert packed.batch_sizes.tolist() == nz  # trimmed to the longest row
    bs_full = np.array(nz + [0] * (c["T"] - len(nz)))
    got = dict(out=packed.data.cpu(), mu=mu.cpu(), lv=lv.cpu(), logits=offl.cpu(), lengths=lengths.cpu().numpy(),
               order=packed.sorted_indices.cpu().numpy(), batch_sizes=bs_full, total=int(packed.data.shape[0]))
    check_against("odd_mean", got, ref)
    assert packed.unsorted_indices[packed.sorted_indices].tolist() == list(range(c["B"]))
    assert torch.equal(packed.data, mu)
    # ... and through the encoder, against the oracle encoder on the reference's packed frames
    h = enc(packed)
    P64 = E._cast(ref["P"], torch.float64)
    with torch.no_grad():
        h64 = O.encoder_forward(P64, ref["packed"]["out"], torch.tensor(nz), ref["ocfg"])
    e = E.rel_err(h, h64)
    print(f"odd_mean encoder(last_hidden): rel_err {e:.2e}")
    assert h.shape == h64.shape and e < HARD, e


def test_generate_edges_small_model():
    from modules import _native as N
    from oracle import abcd_oracle as O
    ref = G.reference("odd_mean")
    c = ref["case"]
    B, T = c["B"], c["T"]
    _, _, dec = _odd_modules(ref)
    feats, spk = ref["feats"].cuda(), ref["speakers"].cuda()
    # a threshold no logit reaches: the packed output is the rectangle, rows in input order
    full, lengths, (mu, lv), offl = dec.generate(feats, T, speaker=spk, mean=True, stop_prob=1.0)
    assert lengths.tolist() == [T] * B and full.batch_sizes.tolist() == [B] * T
    assert full.sorted_indices.tolist() == list(range(B))
    for k, t in (("out", full.data), ("mu", mu), ("lv", lv), ("logits", offl)):
        e = E.rel_err(t, ref["rect"][k])
        print(f"rectangle {k}: rel_err {e:.2e}")
        assert t.shape == ref["rect"][k].shape and e < HARD, (k, e)
    # a threshold every logit exceeds, min_length = 3: the rectangle's first three steps, bit for bit
    cut, lengths, (mu3, _), offl3 = dec.generate(feats, T, speaker=spk, mean=True, stop_prob=0.0, min_length=3)
    assert lengths.tolist() == [3] * B and cut.batch_sizes.tolist() == [B] * 3
    assert torch.equal(cut.data, full.data[:3 * B]) and torch.equal(mu3, mu[:3 * B])
    assert torch.equal(offl3, offl[:3 * B])
    # ... and without min_length every row is one frame
    one, lengths, _, _ = dec.generate(feats, T, speaker=spk, mean=True, stop_prob=0.0)
    assert lengths.tolist() == [1] * B and one.batch_sizes.tolist() == [B] and torch.equal(one.data, full.data[:B])
    # B = 1, T = 1
    p1, l1, (m1, v1), o1 = dec.generate(feats[:1], 1, speaker=spk[:1], mean=True, stop_prob=0.5)
    assert l1.tolist() == [1] and p1.batch_sizes.tolist() == [1] and p1.sorted_indices.tolist() == [0]
    P64 = E._cast(ref["P"], torch.float64)
    with torch.no_grad():
        _, _, o64, (m64, v64), l64 = O.decoder_forward(P64, ref["feats"][:1].double(), [1], ref["ocfg"],
                                                       torch.zeros(1, ref["ocfg"]["F"], dtype=torch.float64),
                                                       speakers=ref["speakers"][:1], train=False)
    for k, a, r in (("out", p1.data, o64), ("mu", m1, m64), ("lv", v1, v64), ("logits", o1, l64)):
        assert a.shape == r.shape and E.rel_err(a, r) < HARD, (k, E.rel_err(a, r))
    assert N.lib().abcd_device_status() == 0
    with pytest.raises(RuntimeError):
        dec.generate(ref["feats"], T, speaker=ref["speakers"])  # CPU tensors are refused


def test_generate_abi_rejects_bad_arguments():
    from modules import _native as N
    from modules.model import _module_pad
    ref = G.reference("odd_mean")
    c = ref["case"]
    B, T = c["B"], c["T"]
    _, _, dec = _odd_modules(ref)
    mp = _module_pad(dec, "decoder")  # the C ABI takes the 16-grid twin
    from modules import padding
    feats = padding.pad_cols(ref["feats"].cuda(), mp.dims.Ddp)
    params = [p.detach() for p in mp.weights(dec._param_list())]
    spk = ref["speakers"].cuda()
    good = mp.twin._cfg_list(1)

    def call(cfg, B=B, T=T, mode=G.MEAN, min_len=1):
        return abi_generate(cfg, params, feats, spk, B, T, mode, None, 0, 0, 0.0, min_len)[0]

    assert call(good) == 0
    assert call(mp.twin._cfg_list(0)) == N.ABCD_EINVAL  # feedback must be 1
    assert call(good, T=0) == N.ABCD_EINVAL
    assert call(good, T=N.GEN_MAX_T + 1, B=1) == N.ABCD_EINVAL  # past the ordering kernel's LDS histogram
    assert call(good, B=0) == N.ABCD_EINVAL
    assert call(good, mode=2) == N.ABCD_EINVAL
    assert call(good, min_len=T + 1) == N.ABCD_EINVAL
    assert N.lib().abcd_decoder_generate_workspace_bytes(N.DecoderCfg(*good), 0, B) == 0
    assert N.lib().abcd_device_status() == 0


def test_generate_philox_seeded():
    """Sample mode with in-kernel Philox noise at c2 widths through generate():
    a seed reproduces its bits, another seed does not, and the lengths follow
    from the returned logits under the stop rule."""
    from modules import noise
    ref = G.reference("c2_mean")
    c = ref["case"]
    B, T = c["B"], c["T"]
    _, _, dec = _bench_modules(ref)
    feats = ref["feats"].cuda()
    saved = noise.get_state()
    try:
        runs = []
        for seed in (7, 7, 8):
            noise.set_mode("philox")
            noise.manual_seed(seed)
            packed, lengths, (mu, lv), offl = dec.generate(feats, T, mean=False, stop_prob=0.5)
            runs.append((packed, lengths, mu, lv, offl))
        torch.cuda.synchronize()
    finally:
        noise.set_state(saved)
    a, b, d = runs
    for x, y in zip((a[0].data, a[1], a[2], a[3], a[4], a[0].sorted_indices),
                    (b[0].data, b[1], b[2], b[3], b[4], b[0].sorted_indices)):
        assert torch.equal(x, y)
    assert a[0].batch_sizes.tolist() == b[0].batch_sizes.tolist()
    n = min(a[0].data.shape[0], d[0].data.shape[0])
    assert not torch.equal(a[0].data[:n], d[0].data[:n])
    assert not torch.equal(a[0].data, a[2])  # a sample, not the mean
    # the stop rule on the returned logits
    packed, lengths, offl = a[0], a[1].cpu().numpy(), a[4].cpu().numpy()
    bs = packed.batch_sizes.numpy()
    off = np.concatenate([[0], np.cumsum(bs)])
    assert int(lengths.sum()) == offl.shape[0] == int(bs.sum())
    assert bs.tolist() == [int((lengths > t).sum()) for t in range(int(lengths.max()))]
    order = packed.sorted_indices.cpu().numpy()
    assert order.tolist() == np.argsort(-lengths, kind="stable").tolist()
    for j, row in enumerate(order.tolist()):
        lg = np.array([offl[off[t] + j] for t in range(int(lengths[row]))])
        assert not (lg[:-1] > 0.0).any(), (row, lg)
        assert lg[-1] > 0.0 or lengths[row] == T, (row, lg)
    assert len(set(lengths.tolist())) > 1


def test_decode_cli_matches_generate(tmp_path):
    import decode
    ckpt = os.path.join(GOLDEN, "ref_ckpt_small.pt")
    out = os.path.join(str(tmp_path), "dec", "out.npz")
    args = [ckpt, "-S", out, "--categories", "0,1,2", "--max_length", "10", "--stop_prob", "0.5", "--min_length", "2"]
    assert decode.main(args) == out
    z = np.load(out, allow_pickle=False)
    assert sorted(z.files) == sorted(["category_ix", "lengths", "batch_sizes", "sorted_indices", "data", "mu",
                                      "log_var", "offset_logits"])
    d = decode.Decoder(ckpt)
    assert not d.decoder.training
    feats = d.feature_sampler.codebook.detach().t()[:3].contiguous()
    spk = None if d.decoder.embed_speaker is None else torch.zeros(3, dtype=torch.int64, device="cuda")
    packed, lengths, (mu, lv), offl = d.decoder.generate(feats, 10, speaker=spk, mean=True, stop_prob=0.5,
                                                         min_length=2)
    assert z["category_ix"].tolist() == [0, 1, 2]
    assert z["lengths"].tolist() == lengths.tolist() and min(z["lengths"]) >= 2
    assert z["batch_sizes"].tolist() == packed.batch_sizes.tolist()
    assert z["sorted_indices"].tolist() == packed.sorted_indices.tolist()
    for k, t in (("data", packed.data), ("mu", mu), ("log_var", lv), ("offset_logits", offl)):
        assert np.array_equal(z[k], t.cpu().numpy()), k
    assert z["data"].shape == (int(z["lengths"].sum()), d.decoder.rnn_cell.cell.input_size)
    assert np.isfinite(z["data"]).all()
    # a rerun keeps the earlier file as .prev and nothing partial
    decode.main(args)
    assert sorted(os.listdir(os.path.dirname(out))) == ["out.npz", "out.npz.prev"]
    assert np.array_equal(np.load(out)["data"], np.load(out + ".prev")["data"])
    with pytest.raises(SystemExit):
        decode.Decoder(os.path.join(GOLDEN, "ref_ckpt_plain.pt"))
