"""The generation cases of ``gen_cases.py``, checked on the CPU: every stop
decision of the float64 reference clears ``STOP_GAP``, the redraw table is what
``find_redraws`` gives today, each case has the property it was built for, and
the numpy stop rule / packing agree with torch's own ``pack_sequence``."""
import numpy as np
import pytest
import torch

import gen_cases as G


@pytest.mark.parametrize("name", list(G.CASES))
def test_stop_gap_holds(name):
    ref = G.reference(name)
    assert ref["gaps"].shape == (ref["case"]["B"],)  # no row excluded
    assert ref["gaps"].min() >= G.STOP_GAP, (name, ref["gaps"].min(), int(ref["gaps"].argmin()))


@pytest.mark.parametrize("name", list(G.CASES))
def test_redraw_table_is_current(name):
    assert G.find_redraws(name) == G.REDRAW.get(name, {})


def _nonadjacent_tie(lengths):
    pos = {}
    for i, l in enumerate(lengths.tolist()):
        pos.setdefault(l, []).append(i)
    return any(max(p) - min(p) > 1 for p in pos.values() if len(p) > 1)


def test_cases_have_what_they_claim():
    L = {n: G.reference(n)["lengths"] for n in G.CASES}
    T = {n: c["T"] for n, c in G.CASES.items()}
    first = {n: G.reference(n)["first"] for n in G.CASES}
    # c2_mean: a stop at step 1, rows that never fire, ties far apart
    assert (L["c2_mean"] == 1).any() and _nonadjacent_tie(L["c2_mean"])
    lg = G.reference("c2_mean")["rect"]["logits"].numpy().reshape(12, 48)
    assert (~(lg > G.reference("c2_mean")["stop_logit"]).any(0)).any()
    assert (L["c2_mean"] == T["c2_mean"]).any()
    # c2gru_sample: the longest row is shorter than T (trailing zeros), several distinct lengths
    assert L["c2gru_sample"].max() < T["c2gru_sample"]
    assert G.reference("c2gru_sample")["batch_sizes"][-1] == 0
    assert len(set(L["c2gru_sample"].tolist())) >= 5 and _nonadjacent_tie(L["c2gru_sample"])
    assert G.reference("c2gru_sample")["eps"].abs().max() > 0  # a sample, not the mean
    # c5gru_mean: min_len lifts rows that fired at the first step; speakers are used
    assert (first["c5gru_mean"] == 0).any() and L["c5gru_mean"].min() == 2 == G.CASES["c5gru_mean"]["min_len"]
    assert L["c5gru_mean"].max() < T["c5gru_mean"]
    assert G.reference("c5gru_mean")["ocfg"]["num_speakers"]
    assert len(set(G.reference("c5gru_mean")["speakers"].tolist())) > 1
    # odd_mean: off the 16-grid, a row that never stops beside rows that stop at once
    o = G.reference("odd_mean")["ocfg"]
    assert any(o[k] % 16 for k in ("Hdec", "Hm", "D", "speaker_dim"))
    assert (L["odd_mean"] == 1).any() and (L["odd_mean"] == T["odd_mean"]).any()
    for n, c in G.CASES.items():
        assert c["B"] <= 65 and c["T"] <= 12


def test_stop_rule():
    nan = float("nan")
    lg = np.array([[0.0, 1.0, nan, 0.5, 0.5],
                   [0.6, 0.0, nan, 0.5, 0.4],
                   [0.9, 0.0, 0.7, 0.5, 0.9]])  # T = 3, B = 5
    lengths, first = G.stop_lengths(lg, 0.5, 1)
    # strict >: 0.5 never fires; NaN never fires; row 4 fires at the last step
    assert lengths.tolist() == [2, 1, 3, 3, 3]
    assert first.tolist() == [1, 0, 2, 2, 2]
    assert G.stop_lengths(lg, 0.5, 2)[0].tolist() == [2, 2, 3, 3, 3]
    assert G.stop_lengths(lg, -np.inf, 3)[0].tolist() == [3, 3, 3, 3, 3]
    assert G.stop_lengths(lg, np.inf, 1)[0].tolist() == [3] * 5


@pytest.mark.parametrize("name", list(G.CASES))
def test_packing_matches_pack_sequence(name):
    """The rows pack_rows selects are torch's PackedSequence of the cut rows."""
    ref = G.reference(name)
    c, lengths = ref["case"], ref["lengths"]
    B, T = c["B"], c["T"]
    rect = ref["rect"]["out"].reshape(T, B, -1)
    seqs = [rect[:int(lengths[b]), b] for b in range(B)]
    pk = torch.nn.utils.rnn.pack_sequence(seqs, enforce_sorted=False)
    # torch sorts by length descending too, but not necessarily stably: compare through each one's own order
    assert pk.batch_sizes.tolist() == [int(x) for x in ref["batch_sizes"] if x > 0]
    assert int(ref["batch_sizes"].sum()) == ref["total"] == pk.data.shape[0]
    assert sorted(ref["order"].tolist()) == list(range(B))
    sl = lengths[ref["order"]]
    assert (np.diff(sl) <= 0).all()
    for l in set(sl.tolist()):  # stable: ties in input order
        assert (np.diff(ref["order"][sl == l]) > 0).all()
    off = np.concatenate([[0], np.cumsum(ref["batch_sizes"])])
    for j, b in enumerate(ref["order"].tolist()):
        for t in range(int(lengths[b])):
            assert torch.equal(ref["packed"]["out"][off[t] + j], rect[t, b])
    if pk.sorted_indices.tolist() == ref["order"].tolist():  # (torch's sort is not promised stable)
        assert torch.equal(pk.data, ref["packed"]["out"])
