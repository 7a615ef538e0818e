"""CPU-side tests of the Griffin-Lim vocoder: the float64 reference the GPU
tests compare against (vocoder_cases.py) does what it claims, and the host
functions of the C ABI (no GPU needed: the library loads here as test_host.py
shows) agree with it."""
import pytest
import torch

import vocoder_cases as V


@pytest.mark.parametrize("framing", list(V.FRAMINGS))
def test_reference_inverts_a_known_phase(framing):
    """n_iter = 0 with the true phase of a toy slice returns the slice: float64
    arithmetic on the float32 log-amplitudes the featuriser writes, within 1e-6
    of the slice's peak."""
    n_fft, hop, window = V.FRAMINGS[framing]
    c = V.make_case(n_fft, hop, window)
    for b in range(c["B"]):
        if not c["samples"][b]:
            continue
        wave, residual = V.griffin_lim_ref(c["A"][b], c["true_phase"][b], n_fft, hop, c["window"], 0, 0.0)
        y = c["slices"][b]
        assert wave.shape == y.shape == (hop * (c["lengths"][b] - 1),)
        e = float((wave - y).abs().max() / y.abs().max())
        print(f"{framing} T={c['lengths'][b]}: |istft - slice| / peak {e:.2e}, residual {residual:.2e}")
        assert e <= 1e-6 and residual <= 1e-6


def test_reference_residual_falls_monotonically():
    n_fft, hop, window = V.FRAMINGS["toy"]
    c = V.make_case(n_fft, hop, window)
    res = [V.reference(c, k, 0.0)[0][1] for k in (1, 2, 4, 8, 32)]
    print("residual after 1, 2, 4, 8, 32 iterations (momentum 0):", ["%.4f" % r for r in res])
    assert all(a > b for a, b in zip(res, res[1:])) and 0.0 < res[-1] < res[0] < 1.0


def test_reference_float32_tracks_float64():
    """The figure the GPU parity bar at 8 iterations is built on."""
    n_fft, hop, window = V.FRAMINGS["toy"]
    c = V.make_case(n_fft, hop, window)
    for mom in (0.0, 0.99):
        w64, r64 = V.reference(c, 8, mom)[0]
        w32, r32 = V.reference(c, 8, mom, dtype=torch.float32)[0]
        e32 = float((w32.double() - w64).abs().max() / w64.abs().max())
        print(f"momentum {mom}: e32 {e32:.2e}, residual {r64:.5f} vs {r32:.5f}")
        assert e32 <= 1e-4 and abs(r64 - r32) <= 1e-4


@pytest.mark.parametrize("T,n_fft,hop,want", [
    (40, 128, 64, 2496), (2, 128, 64, 0), (3, 128, 64, 128), (1, 128, 64, 0),   # 64 = n_fft / 2 is too short
    (200, 256, 128, 25472), (512, 256, 128, 65408),
    (17, 100, 37, 592), (2, 100, 37, 0), (3, 100, 37, 74),
    (17, 101, 50, 800), (2, 101, 50, 0), (3, 101, 50, 100),
    (2, 101, 51, 0),    # 51 samples: the padding behind an odd frame takes n_fft - n_fft / 2 = 51
    (2, 101, 52, 52),
    (4, 64, 64, 192), (2, 64, 64, 64), (1, 64, 64, 0)])
def test_samples_host_function(T, n_fft, hop, want):
    from modules import _native as N
    lib = N.lib()
    got = lib.abcd_griffin_lim_samples(T, n_fft, hop, 1)
    assert got == want == V.samples_of(T, n_fft, hop)
    assert got in (0, hop * (T - 1))
    assert (got == 0) == (hop * (T - 1) <= n_fft - n_fft // 2)
    assert lib.abcd_griffin_lim_samples(T, n_fft, hop, 0) == 0  # center = 0 is out of scope


def test_entry_points_and_dispatch_id():
    from modules import _native as N
    from test_host import header_symbols
    for s in ("abcd_griffin_lim_samples", "abcd_griffin_lim_workspace_bytes", "abcd_griffin_lim"):
        assert s in header_symbols() and s in N.EXPORTED and hasattr(N.lib(), s), s
    assert N.GRIFFIN_LIM == 16 and "griffin_lim" in N.dispatch()
    assert N.lib().abcd_dispatch_count(16) >= 0 and N.lib().abcd_dispatch_count(17) == -1  # TK_N is 17
    # 15 stays unassigned: it read as out of range before the table grew and still does
    assert N.lib().abcd_dispatch_count(15) == -1 and N.lib().abcd_dispatch_name(15) == b""


def test_workspace_query():
    from modules import _native as N
    lib = N.lib()
    base = lib.abcd_griffin_lim_workspace_bytes(4, 40, 128, 64)
    # the phasors and R_prev: T x F complex each per segment
    assert base >= 2 * 4 * 40 * 65 * 8
    assert lib.abcd_griffin_lim_workspace_bytes(8, 40, 128, 64) > base
    assert lib.abcd_griffin_lim_workspace_bytes(4, 80, 128, 64) > base
    assert lib.abcd_griffin_lim_workspace_bytes(1, 1, 128, 64) > 0
    for bad in ((0, 40, 128, 64), (4, 0, 128, 64), (4, 40, 1, 64), (4, 40, 128, 0), (4, 16384, 128, 64),
                (4, 40, 1 << 16, 64)):
        assert lib.abcd_griffin_lim_workspace_bytes(*bad) == 0, bad


def test_vocoder_refuses_cpu_tensors_and_no_centering():
    from modules import data_utils
    with pytest.raises(ValueError, match="centering"):
        data_utils.DeviceVocoder(128, 64, centering=False, device="cpu")
    voc = data_utils.DeviceVocoder(128, 64, device="cpu")
    assert voc.num_samples(40) == 2496 and voc.num_samples(2) == 0
    with pytest.raises(RuntimeError):
        voc((torch.zeros(3, 65), torch.tensor([2, 1])), n_iter=1, seed=0)
