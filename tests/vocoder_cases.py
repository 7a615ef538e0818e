"""Cases and the float64 reference for the Griffin-Lim vocoder tests
(``abcd_griffin_lim``, ``DeviceVocoder``, ``synthesize.py``).

``griffin_lim_ref`` is the definition of include/abcd_hip.h written with
``torch.stft`` / ``torch.istft`` (center, reflect, ``return_complex``), one
segment at a time.  For an odd ``n_fft`` torch's centre padding holds
``n_fft - 1`` samples, one short of the last of the T frames the spectrum has;
the definition pads ``n_fft - n_fft // 2`` behind instead, so there the
reference reflect-pads by hand and calls ``torch.stft(center=False)``.

Bars.  Parity at 0, 1, 2 iterations: 1e-4 of the reference's peak, the
project's standing bar.  At 8 iterations ``max(1e-4, 4 e32)`` with ``e32`` the
error of this same reference run in float32 on the CPU on the same inputs (the
factor 4 covers a different summation order).  Residuals: 1e-4 absolute, and
1e-3 absolute at 32 iterations.
"""
import json
import os

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
TOY_WAV = os.path.join(GOLDEN, "toy_data", "20170806-080002_89.2-94.22.1ch.wav")
EPS = 2.0 ** -15
BAR = 1e-4            # of the reference's peak
RESIDUAL_BAR = 1e-4   # absolute, at the parity settings
CONVERGED_BAR = 1e-3  # absolute, at 32 iterations
LENGTHS = (40, 17, 4, 2, 1)
# (n_fft, hop, window): the toy framing; a hop that does not divide n_fft; an odd n_fft; no overlap
FRAMINGS = {"toy": (128, 64, "hann_window"), "hop37": (100, 37, "hann_window"), "odd": (101, 50, "hann_window"),
            "rect": (64, 64, "ones")}


def window_of(name, n_fft):
    return getattr(torch, name)(n_fft, dtype=torch.float64)


def samples_of(frames, n_fft, hop):
    """S_b, 0 where the reflect padding does not fit."""
    s = hop * (frames - 1)
    return s if s > n_fft - n_fft // 2 else 0


def stft_ref(y, n_fft, hop, window):
    """F x T frames of the S samples, T = S / hop + 1."""
    if n_fft % 2 == 0:
        return torch.stft(y, n_fft, hop_length=hop, window=window, center=True, pad_mode="reflect",
                          return_complex=True)
    yp = torch.nn.functional.pad(y[None, None], (n_fft // 2, n_fft - n_fft // 2), mode="reflect")[0, 0]
    return torch.stft(yp, n_fft, hop_length=hop, window=window, center=False, return_complex=True)


def istft_ref(C, n_fft, hop, window):
    return torch.istft(C, n_fft, hop_length=hop, window=window, center=True, length=hop * (C.shape[1] - 1))


def griffin_lim_ref(A, phase0, n_fft, hop, window, n_iter, momentum, dtype=torch.float64):
    """A, phase0: T x F.  -> (wave S, residual) in ``dtype`` arithmetic."""
    A = A.to(dtype).t().contiguous()
    win = window.to(dtype)
    C = torch.polar(A, phase0.to(dtype).t().contiguous())
    prev = torch.zeros_like(C)
    alpha = momentum / (1.0 + momentum)
    for _ in range(n_iter):
        R = stft_ref(istft_ref(C, n_fft, hop, win), n_fft, hop, win)
        t = R - alpha * prev
        prev = R
        C = A * t / (t.abs() + 1e-16)
    wave = istft_ref(C, n_fft, hop, win)
    residual = (stft_ref(wave, n_fft, hop, win).abs() - A).norm() / A.norm()
    return wave, float(residual)


def magnitudes(logamp, eps=EPS, norm=1.0):
    """float64 magnitudes of the float32 log-amplitudes the kernel reads."""
    return (torch.exp(logamp.double() * norm) - eps).clamp_min(0.0)


def pack(rows):
    """Per-segment T_b x F tensors (length-descending) -> (packed L x F, batch_sizes int64)."""
    lengths = [r.shape[0] for r in rows]
    assert all(a >= b for a, b in zip(lengths, lengths[1:]))
    T = lengths[0]
    bs = torch.tensor([sum(n > t for n in lengths) for t in range(T)], dtype=torch.int64)
    data = torch.cat([torch.stack([rows[b][t] for b in range(int(bs[t]))]) for t in range(T)])
    return data, bs


_wav = None


def toy_wave():
    global _wav
    if _wav is None:
        import scipy.io.wavfile as spw
        _wav = torch.from_numpy(spw.read(TOY_WAV)[1].astype(np.float64))
    return _wav


_cases = {}


def make_case(n_fft, hop, window, lengths=LENGTHS, source="toy", seed=0, norm=1.0):
    """A packed batch with per-segment float64 magnitudes and phases.

    source "toy": segment b is a slice of the toy recording (int16 scale), its
    log-amplitudes those the featuriser writes (no bin is exactly zero), its
    ``true_phase`` the angle of its STFT.  source "random": log-amplitudes ~
    N(3, 2) with no underlying signal.  Segments too short for the reflect
    padding get random frames (the kernel must not read them into anything).
    ``phase`` is a fixed random initial phase in [-pi, pi)."""
    key = (n_fft, hop, window, tuple(lengths), source, seed, norm)
    if key in _cases:
        return _cases[key]
    g = torch.Generator().manual_seed(1000 + seed)
    F = n_fft // 2 + 1
    win = window_of(window, n_fft)
    x_rows, slices, true_phase = [], [], []
    start = 4000
    for T in lengths:
        S = samples_of(T, n_fft, hop)
        if source == "toy" and S:
            wav = toy_wave()
            start = start % (wav.numel() - S)
            y = wav[start:start + S].clone()
            start += 7919
            Z = stft_ref(y, n_fft, hop, win).t()  # T x F
            x_rows.append((torch.log(Z.abs() + EPS) / norm).float())
            slices.append(y)
            true_phase.append(torch.angle(Z).float())
        else:
            x_rows.append((torch.randn(T, F, generator=g, dtype=torch.float64) * 2.0 + 3.0).float() / norm)
            slices.append(None)
            true_phase.append(None)
    phase = [(torch.rand(T, F, generator=g, dtype=torch.float64) * 2 - 1).mul(np.pi).float() for T in lengths]
    data, bs = pack(x_rows)
    c = dict(n_fft=n_fft, hop=hop, window=win, F=F, lengths=list(lengths), B=len(lengths), T=lengths[0],
             L=int(bs.sum()), logamp=data, batch_sizes=bs, phase=phase, phase_packed=pack(phase)[0], slices=slices,
             true_phase=true_phase, A=[magnitudes(x, norm=norm) for x in x_rows], norm=norm,
             samples=[samples_of(T, n_fft, hop) for T in lengths], refs={})
    _cases[key] = c
    return c


def reference(c, n_iter, momentum, dtype=torch.float64, phase=None):
    """Per-segment (wave, residual) of the valid segments, computed once per setting."""
    key = (n_iter, momentum, dtype, None if phase is None else id(phase))
    if key not in c["refs"]:
        ph = c["phase"] if phase is None else phase
        c["refs"][key] = [griffin_lim_ref(c["A"][b], ph[b], c["n_fft"], c["hop"], c["window"], n_iter, momentum, dtype)
                          if c["samples"][b] else None for b in range(c["B"])]
    return c["refs"][key]


def dump(name, rows):
    """Keeps the observed figures when ABCD_VOCODER_DUMP names a JSON file
    (profiles/vocoder_errors.json is written this way)."""
    path = os.environ.get("ABCD_VOCODER_DUMP")
    if not path:
        return
    doc = {}
    if os.path.isfile(path):
        with open(path) as f:
            doc = json.load(f)
    doc[name] = rows
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
