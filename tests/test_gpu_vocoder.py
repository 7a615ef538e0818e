"""The Griffin-Lim vocoder on the GPU: ``abcd_griffin_lim`` through the C ABI
against the float64 reference of ``vocoder_cases.py``, then ``DeviceVocoder``
and the ``synthesize.py`` CLI end to end.

Bars (``vocoder_cases.py``): at 0, 1 and 2 iterations every sample within 1e-4
of the reference's peak; at 8 iterations within ``max(1e-4, 4 e32)`` with e32
the error of the same reference run in float32 on the CPU; residuals within
1e-4 absolute, and within 1e-3 absolute at 32 iterations.  Every observed
figure is printed (``-rA``) and kept with ``ABCD_VOCODER_DUMP``
(profiles/vocoder_errors.json).

Inputs carry NaN column padding, the output rows are NaN before a call: a read
outside a row's F columns or a sample left unwritten shows.
"""
import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest
import torch

import vocoder_cases as V

pytestmark = pytest.mark.gpu

NAN = float("nan")
GOLDEN = V.GOLDEN
PAD_COLS = 3   # NaN columns behind the F real ones of logamp and phase0
PAD_WAVE = 5   # columns of the wave rows behind S_max: never written


def _wide(t, pad=PAD_COLS):
    buf = torch.full((t.shape[0] + 1, t.shape[1] + pad), NAN)
    buf[:t.shape[0], :t.shape[1]] = t
    return buf.cuda()


def _bits(t):
    return t.contiguous().view(torch.int32)


def gl_call(c, n_iter, momentum, phase=None, residual=True, ws="auto", **over):
    """abcd_griffin_lim -> (rc, wave B x (S_max + PAD_WAVE) on the host, residual B or None)."""
    from modules import _native as N
    lib = N.lib()
    F = c["F"]
    a = dict(x=_wide(c["logamp"]), ph=_wide(c["phase_packed"] if phase is None else phase), ld=F + PAD_COLS,
             ldp=F + PAD_COLS, T=c["T"], L=c["L"], B=c["B"], n_fft=c["n_fft"], hop=c["hop"], center=1,
             window=c["window"].float().cuda(), eps=V.EPS, norm=c["norm"])
    a.update(over)
    bs = c["batch_sizes"].contiguous()
    smax = V.samples_of(c["T"], c["n_fft"], c["hop"])
    wave = torch.full((c["B"], smax + PAD_WAVE), NAN, device="cuda")
    res = torch.full((c["B"],), -7.0, device="cuda") if residual else None
    if ws == "auto":
        ws = N.workspace(lib.abcd_griffin_lim_workspace_bytes(c["B"], c["T"], c["n_fft"], c["hop"]), "cuda")
        ws.fill_(0xFF)  # NaN phasors: an entry read without having been written shows
    rc = lib.abcd_griffin_lim(N.ptr(a["x"]), a["ld"], bs.data_ptr(), a["T"], a["L"], a["B"], a["n_fft"], a["hop"],
                              a["center"], N.ptr(a["window"]), a["eps"], a["norm"], N.ptr(a["ph"]), a["ldp"], n_iter,
                              momentum, N.ptr(wave), wave.shape[1], N.ptr(res), N.ptr(ws),
                              0 if ws is None else ws.numel(), N.stream())
    torch.cuda.synchronize()
    return rc, wave.cpu(), None if res is None else res.cpu()


def check_layout(c, wave, res):
    """Zeros behind every segment's samples, zero rows and NaN residuals for the
    segments that are too short, nothing written behind S_max."""
    smax = V.samples_of(c["T"], c["n_fft"], c["hop"])
    assert torch.isnan(wave[:, smax:]).all()
    for b, S in enumerate(c["samples"]):
        assert torch.isfinite(wave[b, :smax]).all(), b
        assert (wave[b, S:smax] == 0).all(), b
        if res is not None:
            assert bool(torch.isnan(res[b])) == (S == 0), (b, res[b])


def errors(c, wave, res, refs):
    """(worst |wave - ref| / ref peak, worst |residual - ref|) over the valid segments."""
    e_w = e_r = 0.0
    for b, S in enumerate(c["samples"]):
        if not S:
            continue
        w64, r64 = refs[b]
        e_w = max(e_w, float((wave[b, :S].double() - w64).abs().max() / w64.abs().max()))
        if res is not None:
            e_r = max(e_r, abs(float(res[b]) - r64))
    return e_w, e_r


def lds_form():
    from modules import _native as N
    return N.dispatch()["griffin_lim"]


@pytest.mark.parametrize("momentum", [0.0, 0.99])
@pytest.mark.parametrize("framing", list(V.FRAMINGS))
def test_parity_against_float64(framing, momentum):
    from modules import _native as N
    n_fft, hop, window = V.FRAMINGS[framing]
    c = V.make_case(n_fft, hop, window)
    assert c["samples"].count(0) >= 1 and len(c["samples"]) - c["samples"].count(0) >= 2
    rows = []
    for n_iter in (0, 1, 2, 8):
        N.lib().abcd_dispatch_reset()
        rc, wave, res = gl_call(c, n_iter, momentum)
        assert rc == 0
        name, count = lds_form()
        assert count == 1 and name.startswith(f"griffin_lim<lds,dft> grid {c['B']} lds "), name
        check_layout(c, wave, res)
        refs = V.reference(c, n_iter, momentum)
        e_w, e_r = errors(c, wave, res, refs)
        bar, e32 = V.BAR, None
        if n_iter == 8:
            r32 = V.reference(c, n_iter, momentum, dtype=torch.float32)
            e32 = max(float((r32[b][0].double() - refs[b][0]).abs().max() / refs[b][0].abs().max())
                      for b in range(c["B"]) if c["samples"][b])
            bar = max(V.BAR, 4.0 * e32)
        print(f"{framing} momentum {momentum} n_iter {n_iter}: |wave - ref| / peak {e_w:.2e} (bar {bar:.2e}"
              + (f", e32 {e32:.2e}" if e32 is not None else "") + f"), |residual - ref| {e_r:.2e}")
        rows.append(dict(framing=framing, momentum=momentum, n_iter=n_iter, wave=e_w, residual=e_r, e32=e32, bar=bar))
        assert e_w <= bar and e_r <= V.RESIDUAL_BAR
        # without the residual the samples keep their bits
        rc, wave2, none = gl_call(c, n_iter, momentum, residual=False)
        assert rc == 0 and none is None and torch.equal(_bits(wave[:, :-PAD_WAVE]), _bits(wave2[:, :-PAD_WAVE]))
    assert N.lib().abcd_device_status() == 0
    V.dump(f"parity_{framing}_m{momentum}", rows)


def test_lds_resident_signal_at_the_config2_framing():
    """n_fft 256, hop 128, T 200: the 101 KiB signal stays in LDS."""
    from modules import _native as N
    c = V.make_case(256, 128, "hann_window", lengths=(200, 150, 37))
    rows = []
    for n_iter, momentum in ((0, 0.0), (2, 0.99)):
        N.lib().abcd_dispatch_reset()
        rc, wave, res = gl_call(c, n_iter, momentum)
        assert rc == 0
        lds = 256 + 3 * 256 * 4 + (128 * 199 + 256) * 4
        assert lds_form() == (f"griffin_lim<lds,dft> grid 3 lds {lds}", 1) and 100 * 1024 < lds < 160 * 1024
        check_layout(c, wave, res)
        e_w, e_r = errors(c, wave, res, V.reference(c, n_iter, momentum))
        print(f"config-2 framing n_iter {n_iter} momentum {momentum}: wave {e_w:.2e} residual {e_r:.2e}")
        rows.append(dict(n_iter=n_iter, momentum=momentum, wave=e_w, residual=e_r))
        assert e_w <= V.BAR and e_r <= V.RESIDUAL_BAR
    assert N.lib().abcd_device_status() == 0
    V.dump("lds_T200", rows)


def test_long_segments_take_the_global_form():
    """T = 512 at the same framing needs 256 KiB: the signal lives in the workspace."""
    from modules import _native as N
    c = V.make_case(256, 128, "hann_window", lengths=(512, 300))
    N.lib().abcd_dispatch_reset()
    rc, wave, res = gl_call(c, 2, 0.99)
    assert rc == 0
    assert lds_form() == (f"griffin_lim<global,dft> grid 2 lds {256 + 3 * 256 * 4}", 1)
    check_layout(c, wave, res)
    e_w, e_r = errors(c, wave, res, V.reference(c, 2, 0.99))
    print(f"T = 512 global form: wave {e_w:.2e} residual {e_r:.2e}")
    V.dump("global_T512", [dict(n_iter=2, momentum=0.99, wave=e_w, residual=e_r)])
    assert e_w <= V.BAR and e_r <= V.RESIDUAL_BAR
    assert N.lib().abcd_device_status() == 0


def test_form_switch_point():
    """At n_fft 256, hop 128 the signal of T = 312 frames is the last that fits
    (256 + 4 * 256 * 4 + 128 * 311 * 4 = 163584 <= 163840 bytes); T = 313 goes
    to the workspace.  Both are checked against the reference."""
    from modules import _native as N
    rows = []
    for T, form in ((312, "lds"), (313, "global")):
        c = V.make_case(256, 128, "hann_window", lengths=(T,))
        N.lib().abcd_dispatch_reset()
        rc, wave, res = gl_call(c, 1, 0.99)
        assert rc == 0
        lds = 256 + 3 * 256 * 4 + ((128 * (T - 1) + 256) * 4 if form == "lds" else 0)
        assert lds_form() == (f"griffin_lim<{form},dft> grid 1 lds {lds}", 1) and lds <= 160 * 1024
        check_layout(c, wave, res)
        e_w, e_r = errors(c, wave, res, V.reference(c, 1, 0.99))
        print(f"T = {T} ({form}): wave {e_w:.2e} residual {e_r:.2e}")
        rows.append(dict(T=T, form=form, wave=e_w, residual=e_r))
        assert e_w <= V.BAR and e_r <= V.RESIDUAL_BAR
    V.dump("switch_point", rows)


@pytest.mark.parametrize("momentum", [0.0, 0.99])
def test_convergence_at_32_iterations(momentum):
    n_fft, hop, window = V.FRAMINGS["toy"]
    c = V.make_case(n_fft, hop, window)
    rc, wave, res = gl_call(c, 32, momentum)
    assert rc == 0
    refs = V.reference(c, 32, momentum)
    rows = []
    for b, S in enumerate(c["samples"]):
        if S:
            print(f"momentum {momentum} T={c['lengths'][b]}: residual {float(res[b]):.5f}, float64 {refs[b][1]:.5f}")
            rows.append(dict(T=c["lengths"][b], residual=float(res[b]), reference=refs[b][1]))
            assert abs(float(res[b]) - refs[b][1]) <= V.CONVERGED_BAR
            assert float(res[b]) < V.reference(c, 1, momentum)[b][1]  # it did converge
    V.dump(f"converged_m{momentum}", rows)


@pytest.mark.parametrize("framing", list(V.FRAMINGS))
def test_true_phase_inversion(framing):
    n_fft, hop, window = V.FRAMINGS[framing]
    c = V.make_case(n_fft, hop, window)
    phase = V.pack([c["phase"][b] if c["true_phase"][b] is None else c["true_phase"][b] for b in range(c["B"])])[0]
    rc, wave, res = gl_call(c, 0, 0.0, phase=phase)
    assert rc == 0
    check_layout(c, wave, res)
    rows = []
    for b, S in enumerate(c["samples"]):
        if S:
            y = c["slices"][b]
            e = float((wave[b, :S].double() - y).abs().max() / y.abs().max())
            print(f"{framing} T={c['lengths'][b]}: |istft - slice| / peak {e:.2e}, residual {float(res[b]):.2e}")
            rows.append(dict(T=c["lengths"][b], wave=e, residual=float(res[b])))
            assert e <= V.BAR and float(res[b]) <= V.RESIDUAL_BAR
    V.dump(f"true_phase_{framing}", rows)


def test_random_spectra():
    """No underlying signal: magnitudes that no STFT has (the projection matters from the first iteration)."""
    c = V.make_case(100, 37, "hann_window", source="random", seed=3, norm=2.0)
    for n_iter, momentum in ((1, 0.0), (2, 0.99)):
        rc, wave, res = gl_call(c, n_iter, momentum)
        assert rc == 0
        check_layout(c, wave, res)
        e_w, e_r = errors(c, wave, res, V.reference(c, n_iter, momentum))
        print(f"random spectra n_iter {n_iter} momentum {momentum}: wave {e_w:.2e} residual {e_r:.2e}")
        assert e_w <= V.BAR and e_r <= V.RESIDUAL_BAR


def test_repeatable_and_independent_of_the_batch():
    n_fft, hop, window = V.FRAMINGS["hop37"]
    c = V.make_case(n_fft, hop, window)
    rc, wave, res = gl_call(c, 3, 0.99)
    rc2, wave2, res2 = gl_call(c, 3, 0.99)
    assert rc == rc2 == 0
    keep = slice(0, wave.shape[1] - PAD_WAVE)
    assert torch.equal(_bits(wave[:, keep]), _bits(wave2[:, keep])) and torch.equal(_bits(res), _bits(res2))
    for b, S in enumerate(c["samples"]):
        one = V.make_case(n_fft, hop, window, lengths=(c["lengths"][b],))
        one = dict(one, logamp=V.pack([_segment(c, b, c["logamp"])])[0], phase_packed=V.pack([c["phase"][b]])[0])
        rc, w1, r1 = gl_call(one, 3, 0.99)
        assert rc == 0
        assert torch.equal(_bits(w1[0, :S]), _bits(wave[b, :S])), b
        assert torch.equal(_bits(r1[:1]), _bits(res[b:b + 1])), b


def _segment(c, b, packed):
    """Segment b's T_b x F rows of a packed tensor."""
    bs = c["batch_sizes"]
    off = np.concatenate([[0], np.cumsum(bs.numpy())])
    return torch.stack([packed[off[t] + b] for t in range(c["lengths"][b])])


CHILD = r"""
import os, sys
assert os.environ["ABCD_GL_LDS"] == "0"
for p in sys.argv[1:4]:
    sys.path.insert(0, p)
import numpy as np, torch
import vocoder_cases as V
import test_gpu_vocoder as G
from modules import _native as N
n_fft, hop, window = V.FRAMINGS["toy"]
c = V.make_case(n_fft, hop, window)
rc, wave, res = G.gl_call(c, 2, 0.99)
assert rc == 0
name = N.dispatch()["griffin_lim"][0]
assert name.startswith("griffin_lim<global,dft>"), name
np.save(sys.argv[4], np.concatenate([wave[:, :-G.PAD_WAVE].numpy().ravel(), res.numpy()]))
print(name)
"""


def test_forced_global_form_agrees(tmp_path):
    """ABCD_GL_LDS=0 in a fresh process (the library reads it per call, but a
    process that has loaded the library keeps its environment)."""
    n_fft, hop, window = V.FRAMINGS["toy"]
    c = V.make_case(n_fft, hop, window)
    rc, wave, res = gl_call(c, 2, 0.99)
    assert rc == 0 and lds_form()[0].startswith("griffin_lim<lds,dft>")
    out = os.path.join(str(tmp_path), "global.npy")
    repo = V.REPO
    env = dict(os.environ, ABCD_GL_LDS="0")
    r = subprocess.run([sys.executable, "-c", CHILD, os.path.join(repo, "tests"), repo,
                        os.path.join(repo, "seq2seq_abcd-vae_amd"), out], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    print("child ran", r.stdout.strip())
    got = torch.from_numpy(np.load(out))
    B, smax = wave.shape[0], wave.shape[1] - PAD_WAVE
    wg, rg = got[:B * smax].reshape(B, smax), got[B * smax:]
    refs = V.reference(c, 2, 0.99)
    e_w, e_r = errors(c, torch.cat([wg, wave[:, smax:]], 1), rg, refs)
    d = max(float((wg[b, :S] - wave[b, :S]).abs().max() / refs[b][0].abs().max())
            for b, S in enumerate(c["samples"]) if S)
    print(f"forced global form: wave {e_w:.2e} residual {e_r:.2e}; against the LDS form {d:.2e}")
    assert e_w <= V.BAR and e_r <= V.RESIDUAL_BAR and d <= V.BAR
    assert torch.equal(torch.isnan(rg), torch.isnan(res))


def test_rejects_bad_arguments():
    from modules import _native as N
    n_fft, hop, window = V.FRAMINGS["toy"]
    c = V.make_case(n_fft, hop, window)
    N.lib().abcd_dispatch_reset()

    def refused(**kw):
        rc, wave, res = gl_call(c, 1, 0.0, **kw)
        assert rc == N.ABCD_EINVAL == 1000, (list(kw), rc)
        assert torch.isnan(wave).all() and (res == -7.0).all()  # nothing written
    refused(center=0)
    refused(ld=c["F"] - 1)
    refused(ldp=c["F"] - 1)
    refused(window=None)
    refused(ws=None)
    refused(ws=torch.empty(8, dtype=torch.uint8, device="cuda"))
    refused(B=c["B"] - 1)
    refused(L=c["L"] + 1)
    refused(x=None)
    refused(ph=None)
    assert lds_form() == ("", 0)  # no launch
    assert N.lib().abcd_griffin_lim(None, 65, c["batch_sizes"].data_ptr(), c["T"], c["L"], c["B"], 128, 64, 1, None,
                                    V.EPS, 1.0, None, 65, -1, 0.0, None, 1, None, None, 0, None) == N.ABCD_EINVAL
    assert N.lib().abcd_device_status() == 0


def test_operator_is_forward_only():
    from modules import ops
    n_fft, hop, window = V.FRAMINGS["toy"]
    c = V.make_case(n_fft, hop, window)
    x, ph, win = c["logamp"].cuda(), c["phase_packed"].cuda(), c["window"].float().cuda()
    waves, res = ops.griffin_lim(x, c["batch_sizes"], win, ph, hop, V.EPS, 1.0, 2, 0.99, True)
    rc, wave, res0 = gl_call(c, 2, 0.99)
    assert waves.shape == (c["B"], V.samples_of(c["T"], n_fft, hop))
    assert torch.equal(_bits(waves.cpu()), _bits(wave[:, :-PAD_WAVE]))
    assert torch.equal(_bits(res.cpu()), _bits(res0))
    with pytest.raises(RuntimeError, match="forward-only"):
        ops.griffin_lim(x.clone().requires_grad_(True), c["batch_sizes"], win, ph, hop, V.EPS, 1.0, 2, 0.99, True)
    with pytest.raises(ValueError):
        ops.griffin_lim(x[:, :-1], c["batch_sizes"], win, ph[:, :-1], hop, V.EPS, 1.0, 2, 0.99, True)


# ----------------------------------------------------------------------------
# end to end
# ----------------------------------------------------------------------------
def test_featurize_vocode_featurize():
    """DeviceFeaturizer on toy segments, DeviceVocoder with 32 iterations,
    DeviceFeaturizer again: the re-analysed spectra reproduce the reported
    residual (1e-4 absolute, the residual bar), the same seed the same bits."""
    from modules import data_utils
    n_fft, hop = 128, 64
    wav = V.toy_wave().float().numpy()
    lens = [hop * (T - 1) for T in (40, 17, 9)]
    segs = [wav[10000 + 3000 * i:10000 + 3000 * i + n] for i, n in enumerate(lens)]
    feat = data_utils.DeviceFeaturizer(n_fft, hop)
    voc = data_utils.DeviceVocoder(n_fft, hop)
    data, bs, _ = feat(segs)
    waves, n_samples, res = voc((data, bs), n_iter=32, seed=5)
    assert n_samples.tolist() == lens and waves.shape == (3, lens[0]) and res.shape == (3,)
    again, bs2, _ = feat([waves[b, :n].cpu().numpy() for b, n in enumerate(lens)])
    assert torch.equal(bs, bs2)
    A, A2 = V.magnitudes(data.cpu()), V.magnitudes(again.cpu())
    off = np.concatenate([[0], np.cumsum(bs.numpy())])
    for b, T in enumerate((40, 17, 9)):
        rows = torch.tensor([off[t] + b for t in range(T)])
        r = float((A2[rows] - A[rows]).norm() / A[rows].norm())
        print(f"T={T}: reported residual {float(res[b]):.5f}, re-analysed {r:.5f}")
        assert abs(r - float(res[b])) <= V.RESIDUAL_BAR and 0.0 < r < 0.5
    w2, _, r2 = voc(torch.nn.utils.rnn.PackedSequence(data, bs), n_iter=32, seed=5)
    assert torch.equal(_bits(waves), _bits(w2)) and torch.equal(_bits(res), _bits(r2))
    w3, _, r3 = voc((data, bs), n_iter=32, seed=6, residual=False)
    assert not torch.equal(waves, w3) and torch.isnan(r3).all()
    with pytest.raises(ValueError):
        data_utils.DeviceVocoder(n_fft, hop, centering=False)


def _check_dir(out, z, n_fft, hop, float32=False):
    import synthesize
    df = pd.read_csv(os.path.join(out, "synthesis.csv"))
    assert list(df.columns) == list(synthesize.COLUMNS)
    n = len(z["category_ix"])
    assert df["index"].tolist() == list(range(n)) and df["category_ix"].tolist() == z["category_ix"].tolist()
    assert df["frames"].tolist() == z["lengths"].tolist()
    want = [V.samples_of(int(T), n_fft, hop) for T in z["lengths"]]
    assert df["samples"].tolist() == want
    wavs = sorted(f for f in os.listdir(out) if f.endswith(".wav"))
    assert wavs == sorted(f"category_{k}.wav" for k, s in zip(z["category_ix"], want) if s)
    import scipy.io.wavfile as spw
    for _, row in df.iterrows():
        if row["samples"] == 0:
            assert pd.isna(row["path"]) and np.isnan(row["residual"]) and row["clipped_samples"] == 0
            continue
        assert row["path"] == f"category_{row['category_ix']}.wav" and 0.0 <= row["residual"] < 1.0
        fs, w = spw.read(os.path.join(out, row["path"]))
        assert fs == 16000 and w.shape == (row["samples"],) and row["samples"] == hop * (row["frames"] - 1)
        assert w.dtype == (np.float32 if float32 else np.int16)
        if not float32:  # a saturated sample sits on a limit (so may, rarely, one that was not clipped)
            assert row["clipped_samples"] <= int(((w == 32767) | (w == -32768)).sum())
    return df, wavs


def test_synthesize_cli_on_decoded_toy_checkpoint(tmp_path):
    import decode
    import synthesize
    ckpt = os.path.join(GOLDEN, "ref_ckpt_small.pt")
    n_fft, hop = 128, 64  # 0.008 s and 0.004 s at 16 kHz
    # the offset predictor stops the sequences where it likes (frames of 1 and 2 are too short to invert)
    free = os.path.join(str(tmp_path), "free.npz")
    decode.main([ckpt, "-S", free, "--categories", "0,1,2,3", "--max_length", "12", "--min_length", "1"])
    out = os.path.join(str(tmp_path), "free")
    assert synthesize.main([free, "16000", "1.0", "-S", out]) == out
    z = np.load(free, allow_pickle=False)
    df, _ = _check_dir(out, z, n_fft, hop)
    print("free-running lengths", z["lengths"].tolist(), "residuals", df["residual"].tolist())
    # every sequence 12 frames long: four wavs
    full = os.path.join(str(tmp_path), "full.npz")
    decode.main([ckpt, "-S", full, "--categories", "3,0,2,1", "--max_length", "12", "--stop_prob", "1.0"])
    z = np.load(full, allow_pickle=False)
    assert z["lengths"].tolist() == [12] * 4
    out = os.path.join(str(tmp_path), "full")
    synthesize.main([full, "16000", "1.0", "-S", out, "--seed", "1"])
    df, wavs = _check_dir(out, z, n_fft, hop)
    assert len(wavs) == 4 and (df["samples"] == hop * 11).all()
    print("12-frame residuals", df["residual"].tolist(), "clipped", df["clipped_samples"].tolist())
    read = lambda d, f: open(os.path.join(d, f), "rb").read()  # noqa: E731
    first = {f: read(out, f) for f in wavs}
    # the same seed: byte-identical wavs, the earlier ones kept as .prev; another seed: other wavs
    synthesize.main([full, "16000", "1.0", "-S", out, "--seed", "1"])
    assert all(read(out, f) == first[f] == read(out, f + ".prev") for f in wavs)
    assert not [f for f in os.listdir(out) if f.endswith(".partial")]
    other = os.path.join(str(tmp_path), "other")
    synthesize.main([full, "16000", "1.0", "-S", other, "--seed", "2", "--field", "data"])
    assert all(read(other, f) != first[f] for f in wavs)
    # float32 output, the amplitudes a data_normalizer of 2 implies
    fl = os.path.join(str(tmp_path), "float")
    synthesize.main([full, "16000", "1.0", "-S", fl, "--seed", "1", "--float32"])
    _check_dir(fl, z, n_fft, hop, float32=True)
    import scipy.io.wavfile as spw
    for f in wavs:
        w16, clipped = synthesize.to_int16(spw.read(os.path.join(fl, f))[1])
        assert np.array_equal(w16, spw.read(os.path.join(out, f))[1])
        assert clipped == int(df.loc[df["path"] == f, "clipped_samples"].iloc[0])
    with pytest.raises(SystemExit):
        synthesize.main([full, "16000", "1.0", "-S", fl, "--fft_no_centering"])
    with pytest.raises(SystemExit):
        synthesize.main([full, "32000", "1.0", "-S", fl])  # 256-sample frames: not this model's 65 bins
    assert synthesize.to_int16(np.array([4e4, -4e4, 1.4, -32768.2]))[0].tolist() == [32767, -32768, 1, -32768]
    assert synthesize.to_int16(np.array([4e4, -4e4, 1.4, -32768.2]))[1] == 2
