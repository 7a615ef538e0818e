"""abcd_fill_dropout and abcd_fill_normal against the numpy Philox4x32-10 of
``tests/sampler_cases.py`` (which test_sampler_cases_cpu.py pins to
Random123's known answers).

The kernels draw element i of stream (seed, offset) from the counter
(low, high word of offset + i, 0, 0) under the key (low, high word of seed);
dropout keeps where u01(word 0) <= 1 - p, the normal is the Box-Muller of
u01(word 0) and u01(word 1).  u01(x) = ((x >> 8) + 1) 2^-24 is exact in fp32,
so the keep pattern is compared exactly; the normal, which goes through the
device's fast log and cosine, to 1e-4 absolute -- a bound that separates the
right stream from any wrong word, counter or transform (all O(1) off), not a
claim about the intrinsics (the observed maximum is printed and recorded).
The seed has a non-zero high word, and one offset puts the carry of
offset + i into the counter's high word inside the buffer.

The C ABI has no one-thread path to the raw Philox words, so Random123's
known answers are checked on the numpy side only.
"""
import numpy as np
import pytest
import torch

import sampler_cases as S
from edge_cases import dump_observed

pytestmark = pytest.mark.gpu

SEED = 0x9E3779B97F4A7C15
SENT = 12345.0
GUARD = 4
CARRY = 2 ** 32 - 5  # offset + 5 is the first index with a non-zero high word


def _fill(kind, n, seed, offset, p=None):
    """n values from the device into a NaN-filled buffer with GUARD sentinels after them; (return code, values)."""
    from modules import _native as N
    buf = torch.full((n + GUARD,), float("nan"), device="cuda")
    buf[n:] = SENT
    if kind == "normal":
        rc = N.lib().abcd_fill_normal(N.ptr(buf), n, seed, offset, N.stream())
    else:
        rc = N.lib().abcd_fill_dropout(N.ptr(buf), n, p, seed, offset, N.stream())
    torch.cuda.synchronize()
    assert bool((buf[n:] == SENT).all()), "written past element n - 1"
    return rc, buf[:n].cpu().numpy()


@pytest.mark.parametrize("offset", [0, 12345, CARRY])
@pytest.mark.parametrize("n", [1, 1000, 1048579])
@pytest.mark.parametrize("p", [0.0, 0.2, 0.5])
def test_fill_dropout_matches_numpy_stream(p, n, offset):
    rc, got = _fill("dropout", n, SEED, offset, p)
    assert rc == 0
    keep, val = S.dropout(SEED, S.indices(offset, n), p)
    assert np.array_equal(got != 0, keep), f"{int((( got != 0) != keep).sum())} of {n} keep decisions differ"
    kept = got[keep]
    assert np.all(np.abs(kept.astype(np.float64) - val) <= np.spacing(np.float32(val)))
    assert len(np.unique(kept)) <= 1
    if p == 0.0:
        assert np.all(got == 1.0)
    elif n >= 1000:
        assert abs(keep.mean() - (1.0 - p)) < 0.05


@pytest.mark.parametrize("kind", ["dropout", "normal"])
def test_offset_is_a_shift_of_the_counter(kind):
    """fill(n, offset = k) equals fill(n + k, 0)[k:] bit for bit, also across the carry."""
    n, k = 5000, 12345
    for base in (0, CARRY - k):
        _, whole = _fill(kind, n + k, SEED, base, 0.2)
        _, part = _fill(kind, n, SEED, base + k, 0.2)
        assert np.array_equal(whole[k:].view(np.uint32), part.view(np.uint32)), (kind, base)
        assert not np.array_equal(whole[:n], part)


def test_fill_dropout_argument_errors():
    from modules import _native as N
    for p in (1.0, -0.1, float("nan")):
        rc, got = _fill("dropout", 16, SEED, 0, p)
        assert rc == N.ABCD_EINVAL, (p, rc)
        assert np.isnan(got).all()  # nothing was launched


@pytest.mark.parametrize("offset", [0, CARRY])
def test_fill_normal_matches_numpy_stream(offset, record_property):
    n = 1 << 20
    rc, got = _fill("normal", n, SEED, offset)
    assert rc == 0
    assert np.isfinite(got).all()
    idx = S.indices(offset, n)
    want = S.normal(SEED, idx)
    err = np.abs(got.astype(np.float64) - want)
    worst = float(err.max())
    print(f"fill_normal offset {offset}: max abs err {worst:.3e} at |z| = {abs(want[err.argmax()]):.3e}, "
          f"mean {got.mean():.2e} std {got.std():.6f}")
    rows = [dict(what="abcd_fill_normal against the float64 Box-Muller of the numpy uniforms", n=n, offset=offset,
                 max_abs_err=worst)]
    record_property("parity_errors", rows)
    dump_observed(f"philox-normal-off{offset}", rows)
    # the wrong streams this bound tells apart: the low counter word only (no carry), swapped words, another key word
    w = S.words(SEED, idx)
    swapped = np.sqrt(-2.0 * np.log(S.u01(w[1]))) * np.cos(2.0 * np.pi * S.u01(w[0]))
    assert np.abs(swapped - want).max() > 1.0
    assert np.abs(S.normal(SEED & 0xFFFFFFFF, idx) - want).max() > 1.0
    if offset:
        assert np.abs(S.normal(SEED, idx & S._M32) - want)[5:].max() > 1.0
    assert worst <= 1e-4, worst
    _, other = _fill("normal", 4096, SEED + 1, offset)
    assert not np.array_equal(other, got[:4096]) and np.abs(other - got[:4096]).max() > 1.0
    _, again = _fill("normal", 4096, SEED, offset)
    assert np.array_equal(again.view(np.uint32), got[:4096].view(np.uint32))
