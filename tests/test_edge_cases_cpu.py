"""The conditions that make tests/test_gpu_edges.py meaningful (no GPU).

* every case of ``edge_cases.CASES`` has the batch-size profile its name
  claims (the group / tile boundary it was built to hit);
* the unit the GPU tests measure in -- the fp32 oracle against the float64
  oracle -- is honest-fp32 small: <= 1e-5 in ``block_err`` and ``rel_err`` on
  every gradient (measured 4.4e-6 / 3.1e-6); loss, em and off <= 1e-6
  relative, the KL within 4 ulp of each of the two sums it is the difference of;
* exactly the gradients listed in ``ZERO_GRADS`` are identically zero in
  float64 (the GPU must then produce exact zeros);
* the argmax comparison is fair: in float64 every row's top-2 logit gap is
  >= 1e-3, ten times the 1e-4 logit tolerance, and the table of redrawn rows
  that achieves it is what ``edge_cases.find_redraws`` gives;
* the fast tanh form the kernels use moves, in the fp32 oracle, the tensors
  whose R test_gpu_edges.py raises.
"""
import math

import pytest
import torch

import edge_cases as E

C2 = ("c2", "c2gru")
ARGMAX_WIDTHS = [(c, w) for c in E.CASES for w in C2] + [(c, "c5gru") for c in ("b33", "b97steep", "b160")]


def _bs(case):
    lengths = E.CASES[case]
    return [sum(1 for n in lengths if n > t) for t in range(lengths[0])]


def _groups(B, rows):
    return -(-B // rows)


def test_cases_are_sorted_and_short():
    assert list(E.CASES) == ["b32eq", "b1t7", "b1t1", "b31tail", "b33", "b65", "b97steep", "b160", "b256t3"]
    for case, lengths in E.CASES.items():
        assert lengths == sorted(lengths, reverse=True), case
        assert 1 <= min(lengths) and max(lengths) <= 12, case
        cfg = E.config("c2", len(lengths))
        batch, noise = E.make_batch(lengths, cfg, E.SEED)
        assert batch["batch_sizes"].tolist() == _bs(case), case
        L = sum(lengths)
        assert batch["data"].shape == (L, cfg["F"]) and noise["eps"].shape == (L, cfg["F"])
        assert float(batch["is_offset"].sum()) == len(lengths)  # one offset per segment, on its last frame
        assert noise["feat"].shape == (len(lengths), cfg["K"])


def test_case_geometry():
    bs = {c: _bs(c) for c in E.CASES}
    assert bs["b1t1"] == [1]                                          # B = 1, T = 1
    assert bs["b1t7"] == [1] * 7                                      # B = 1, below every row group
    assert bs["b32eq"] == [32] * 5                                    # exactly one 32-row group, no shrink
    assert bs["b33"] == [33] + [32] * 5                               # one row past the group, for one step
    assert bs["b31tail"] == [31, 8, 7, 6, 5, 4, 3, 2, 1]              # below one group, length-1 segments, to 1 row
    b = bs["b65"]
    assert b[0] == 65 and len(b) == 12 and _groups(65, 64) == 2 and _groups(65, 32) == 3
    for edge in (64, 32, 16):                                         # both sides of each boundary are visited
        assert any(x > edge for x in b) and any(x <= edge for x in b), edge
    assert b == [65, 65, 64, 64, 64, 33, 33, 17, 17, 17, 3, 3]
    assert bs["b97steep"] == [97] + [1] * 11                          # 4 groups of 32, all but row 0 end at once
    b = bs["b160"]
    assert b[0] == 160 and len(b) == 8 and b[-1] >= 1
    assert _groups(160, 32) == 5 and _groups(160, 32) % 8 != 0 and _groups(160, 64) == 3
    assert all(x > y for x, y in zip(b, b[1:]))                       # ragged: shrinks at every step
    assert any(x % 64 for x in b) and b[-1] < 32                      # ragged tiles, down to part of one group
    b = bs["b256t3"]
    assert b[0] == 256 and len(b) == 3
    assert _groups(256, 32) % 8 == 0 and _groups(256, 16) % 8 == 0    # the ngroups % 8 == 0 mapping
    assert b[0] > b[1] > b[2] >= 1
    # a group whose rows have all ended while the others run on
    assert _groups(bs["b97steep"][1], 32) < _groups(97, 32) and _groups(bs["b65"][-1], 32) < _groups(65, 32)


def test_block_err_sees_one_wrong_tile():
    g = torch.Generator().manual_seed(0)
    ref = torch.randn(40, 50, generator=g, dtype=torch.float64)
    ref[16:32, 32:48] *= 1e-3                       # a quiet tile
    a = ref.clone()
    a[20, 40] += 1e-4 * float(ref[16:32, 32:48].abs().max())
    assert E.rel_err(a, ref) < 1e-7                 # invisible in units of the tensor's max
    got = E.block_err(a, ref, floor=1e-4)
    assert abs(got - 1e-4) < 1e-9
    # the floor keeps a near-zero block from dividing by nothing
    lo = 1e-2 * float(ref.abs().max())
    assert abs(E.block_err(a, ref) - 1e-4 * float(ref[16:32, 32:48].abs().max()) / lo) < 1e-12
    assert E.block_err(ref, ref) == 0.0
    v = torch.arange(1.0, 36.0, dtype=torch.float64)  # 1-D: one row of 16-wide blocks, zero-padded
    w = v.clone()
    w[34] += 0.35
    assert abs(E.block_err(w, v) - 0.01) < 1e-12
    assert E.block_err(torch.zeros(3, 3), torch.zeros(3, 3)) == 0.0
    # slack: an elementwise allowance taken off |a - ref| (the stored parameter's half-ulp)
    p = torch.full((4, 4), 0.75, dtype=torch.float64)
    sl = E.store_slack(p)
    assert torch.equal(sl, p * 2.0 ** -24)
    d = torch.full((4, 4), 1e-4, dtype=torch.float64)
    assert E.rel_err(d + 0.9 * sl, d, slack=sl) == 0.0 and E.block_err(d + 0.9 * sl, d, slack=sl) == 0.0
    assert abs(E.rel_err(d + 3 * sl, d, slack=sl) - 2 * float(sl[0, 0]) / 1e-4) < 1e-12


@pytest.mark.parametrize("widths", C2)
@pytest.mark.parametrize("case", list(E.CASES))
def test_fp32_oracle_vs_float64(case, widths):
    ref = E.reference(case, widths)
    r32, r64 = ref["r32"], ref["r64"]
    assert all(g.dtype == torch.float64 for g in r64["grads"].values())
    assert all(g.dtype == torch.float32 for g in r32["grads"].values())
    a, b = float(r32["out"]["loss"]), float(r64["out"]["loss"])
    assert abs(a - b) <= 1e-6 * abs(b), ("loss", a, b)
    # the terms, in units of the sum they enter the loss through ...
    total = abs(float(r64["out"]["em"] + r64["out"]["off"] + r64["out"]["kl"]))
    for k in ("em", "off", "kl"):
        a, b = float(r32["out"][k]), float(r64["out"][k])
        print(case, widths, k, "fp32 vs float64: %.2e relative" % (abs(a - b) / abs(b)))
        assert abs(a - b) <= 1e-6 * total, (k, a, b)
    # ... em and off also on their own; the KL against its own cancellation:
    # it is sum(q log q) - sum(q E[log pi]) plus a prior term scaled by B / N,
    # two sums of magnitude B ln K each (q near uniform at init, E[log pi] ~
    # -ln K) whose difference is ~10x smaller, so its own relative error
    # reaches 3e-6.  Each sum is granted 4 fp32 ulp (2^-22) of its magnitude.
    for k in ("em", "off"):
        a, b = float(r32["out"][k]), float(r64["out"][k])
        assert abs(a - b) <= 1e-6 * abs(b), (k, a, b)
    B, K = ref["cfg"]["B"], ref["cfg"]["K"]
    a, b = float(r32["out"]["kl"]), float(r64["out"]["kl"])
    assert abs(a - b) <= 2.0 ** -22 * 2 * B * math.log(K), ("kl", a, b, 2.0 ** -22 * 2 * B * math.log(K))
    err = E.oracle_errors(ref)
    worst = {k: v for k, v in err.items() if k.startswith("g/")}
    print(case, widths, "worst rel_err %.2e block_err %.2e" % (max(v[0] for v in worst.values()),
                                                                max(v[1] for v in worst.values())))
    for k, (rel, blk) in worst.items():
        assert rel <= 1e-5 and blk <= 1e-5, (k, rel, blk)
    zero = {k for k, g in r64["grads"].items() if not g.any()}
    assert zero == E.ZERO_GRADS.get(case, set()), zero
    assert all(torch.isfinite(g).all() for g in r64["grads"].values())


@pytest.mark.parametrize("case,widths", ARGMAX_WIDTHS)
def test_argmax_is_a_fair_test(case, widths):
    logits = E.logits64(case, widths, E.REDRAW.get((case, widths)))
    assert logits.dtype == torch.float64 and logits.shape == (len(E.CASES[case]), E.config(widths, 1)["K"])
    assert E.top2_gap(logits) >= E.ARGMAX_GAP, E.top2_gap(logits)
    # the committed table is what the search gives today (no stale or needless entry)
    assert E.find_redraws(case, widths) == E.REDRAW.get((case, widths), {})


def test_fast_tanh_form_moves_emission_w2(monkeypatch):
    """What test_gpu_edges.R_TENSOR is attributed to, checked without a GPU.
    The kernels' tanh is ftanh (abcd_common.h): 1 - 2 / (1 + e^2x), whose error
    is absolute (~1e-7) where torch's is relative.  The fp32 oracle run with
    that form, against the same fp32 oracle with torch's tanh (same machine,
    same summation order: the difference is the tanh form alone), moves the
    tensors that read the emission MLP's hidden activation -- mu, and the
    second layer's weight and bias gradients -- by what the GPU shows against
    float64 (1.1e-6, 5.4e-6 and 2.7e-6 in profiles/parity_errors.json), several
    times the fp32 oracle's own error, and stays far under the hard 1e-4."""
    em = "decoder/emission_sampler.to_parameters.mlps.%d.whole_network.2.%s"

    def fast_tanh(x):
        return 1.0 - 2.0 / (1.0 + torch.exp(2.0 * x))

    def shifted(case):
        ref = E.reference(case, "c2")
        with monkeypatch.context() as m:
            m.setattr(torch, "tanh", fast_tanh)
            fast = E.oracle32(ref["ocfg"], ref["P"], ref["batch"], ref["noise"], E.N_DATA)
        return ref, fast

    ref, fast = shifted("b1t1")  # one row: the same sums whatever the thread count
    for head in (0, 1):
        k = em % (head, "weight")
        shift = E.rel_err(fast["grads"][k], ref["r32"]["grads"][k])
        e32 = E.rel_err(ref["r32"]["grads"][k], ref["r64"]["grads"][k])
        print(k, "shift %.2e e32 %.2e" % (shift, e32))
        assert 5e-7 <= shift <= 5e-6 and shift >= 3 * e32, (k, shift, e32)
    ref, fast = shifted("b65")
    k = em % (1, "bias")  # a cancelling sum over 445 frames; its quietest 16-wide block is ~1% of the tensor's max
    shift = E.block_err(fast["grads"][k], ref["r32"]["grads"][k])
    print(k, "shift %.2e" % shift)
    assert 1e-6 <= shift <= 2e-5, shift
    assert E.rel_err(fast["grads"][k], ref["r32"]["grads"][k]) <= 5e-7
    ref, fast = shifted("b33")
    shift = E.block_err(fast["out"]["mu"], ref["r32"]["out"]["mu"])
    print("mu shift %.2e" % shift)
    assert 5e-7 <= shift <= 1e-5, shift
