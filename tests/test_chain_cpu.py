"""The category-sequence HMM, checked on the CPU: the float64 oracle of
``chain_cases.py`` against brute-force enumeration and against the pairwise
posterior it generalises, its EM, the generators' "decided" cap; the new entry
points' surface (header, binding, plan, workspace query, host-side argument
checks, custom op); ``split_sequences`` and ``sequence.py``'s arguments."""
import ctypes
import os

import numpy as np
import pandas as pd
import pytest
import torch

import chain_cases as C
import pairwise_cases as PW

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ANN = os.path.join(GOLDEN, "toy_data", "annotation_20170806-080002_89.2-94.22.csv")


def test_oracle_is_brute_force_enumeration():
    g = np.random.default_rng(11)
    K = 3
    for T in (1, 2, 3, 4, 5):
        for trial in range(3):
            trans, init = C.draw_chain(K, g, zeros=trial == 2)
            with np.errstate(divide="ignore"):
                lt, li = np.log(trans), np.log(init)
            sc = -4.0 * g.random((T, K))
            bf = C.brute_force(sc, lt, li)
            r = C.oracle(sc, [0, T], lt, li)
            assert abs(r["log_evidence"][0] - bf["log_evidence"]) <= 1e-12 * abs(bf["log_evidence"])
            assert np.abs(r["gamma"] - bf["gamma"]).max() <= 1e-12
            assert np.abs(r["trans_counts"] - bf["trans_counts"]).max() <= 1e-12
            assert np.abs(r["init_counts"] - bf["init_counts"]).max() <= 1e-12
            assert abs(r["path_score"][0] - bf["path_score"]) <= 1e-12 * abs(bf["path_score"])
            assert r["path"].tolist() == bf["path"].tolist()
            assert abs(r["gamma"].sum() - T) <= 1e-12 and abs(r["trans_counts"].sum() - (T - 1)) <= 1e-12
    # ties (small integers: every sum is exact): the lowest index wins at the final state and at every back-pointer
    lt = np.zeros((K, K))
    li = np.zeros(K)
    sc = np.array([[0.0, 0.0, -1.0], [-1.0, 0.0, 0.0], [0.0, -2.0, 0.0], [0.0, 0.0, 0.0]])
    for T in (1, 2, 3, 4):
        bf, r = C.brute_force(sc[:T], lt, li), C.oracle(sc[:T], [0, T], lt, li)
        assert r["path"].tolist() == bf["path"].tolist() == [0, 1, 0, 0][:T]
        assert not r["decided"][0]
    # several sequences, an empty one among them, are the single sequences side by side
    sc = -3.0 * g.random((7, K))
    trans, init = C.draw_chain(K, g)
    with np.errstate(divide="ignore"):
        lt, li = np.log(trans), np.log(init)
    r = C.oracle(sc, [0, 3, 3, 7], lt, li)
    a, b = C.oracle(sc[:3], [0, 3], lt, li), C.oracle(sc[3:], [0, 4], lt, li)
    assert r["log_evidence"].tolist() == [a["log_evidence"][0], 0.0, b["log_evidence"][0]] and np.isnan(r["path_score"][1])
    assert np.abs(r["trans_counts"] - a["trans_counts"] - b["trans_counts"]).max() <= 1e-15
    assert r["path"].tolist() == a["path"].tolist() + b["path"].tolist()
    lj = C.path_log_joint(r["path"], sc, [0, 3, 3, 7], lt, li)
    assert np.abs(lj[[0, 2]] - r["path_score"][[0, 2]]).max() <= 1e-12
    # exclusions
    inf = np.inf
    sc = np.array([[0.0, np.nan, -1.0], [np.nan, np.nan, inf], [0.0, 0.0, 0.0]])
    r = C.oracle(sc, [0, 1, 3], np.zeros((K, K)) - np.log(K), np.zeros(K) - np.log(K))
    assert r["gamma"][0, 1] == 0 and r["log_evidence"][1] == -inf and r["path"].tolist() == [0, -1, -1]
    assert (r["gamma"][1:] == 0).all() and r["path_score"][1] == -inf and r["trans_counts"].sum() == 0
    assert abs(r["init_counts"].sum() - 1.0) <= 1e-12


def test_oracle_em_never_decreases_its_objective():
    c = C.case(5, "many")
    u = np.full((5, 5), -np.log(5.0), dtype=np.float32)
    objs = C.em_reference(c["score"].numpy(), c["seq_off"].numpy(), u, u[0], 10, 0.2)
    assert len(objs) == 11
    # the parameters pass through float32 after every M-step: each is normalised to 2^-24 relative only, which
    # moves the objective by at most that times the number of transitions and initial states
    slack = 2.0 ** -23 * float(c["seq_off"][-1])
    assert (np.diff(objs) >= -slack).all() and objs[-1] > objs[0] + 1.0


def test_context_free_model_is_the_pairwise_posterior():
    for B, P in ((5, 16), (33, 65)):
        c = PW.posterior_inputs(B, P)
        s = -(c["em"].double() + c["off"].double()).numpy()
        lw = c["lw"].double().numpy()
        p = lw - (lw.max() + np.log(np.exp(lw - lw.max()).sum()))       # log softmax
        m = s.max(1)
        r = C.oracle(s - m[:, None], [0, 1, B], np.tile(p, (P, 1)), p)
        ref = c["ref"]
        assert np.abs(r["gamma"] - ref["resp"]).max() <= 1e-12
        assert (r["path"] == ref["best"]).all()
        total = r["log_evidence"].sum() + m.sum() + B * (lw.max() + np.log(np.exp(lw - lw.max()).sum()))
        assert abs(total - ref["log_evidence"].sum()) <= 1e-12 * abs(ref["log_evidence"].sum())


def test_generated_cases_are_mostly_decided():
    total = undecided = 0
    for K, kind in C.case_ids():
        c = C.case(K, kind)
        lens = np.asarray(c["lengths"])
        assert set(lens.tolist()) <= set(C.LENGTHS) and c["score"].shape == (lens.sum(), K + C.PAD)
        assert torch.isnan(c["score"][:, K:]).all() and torch.isnan(c["log_trans"][:, K:]).all()
        if lens.sum():
            assert float(c["score"][:, :K].max(1).values.abs().max()) == 0.0     # rows normalised to a maximum of 0
        if K == 1024:
            assert lens.sum() <= 64
        live = lens > 0
        assert np.isfinite(c["ref"]["log_evidence"]).all()      # the true states follow the chain: no dead sequence
        total += int(live.sum())
        undecided += int((~c["ref"]["decided"][live]).sum())
        if kind == "many":
            assert len(lens) == 2 * C.plan(K, len(lens))[1] + 1
    print(f"undecided sequences: {undecided} of {total}")
    assert undecided <= C.UNDECIDED_CAP * total
    assert any(np.isinf(c["log_trans"][:, :c["K"]].numpy()).any() for c in (C.case(64, "one"), C.case(128, "three")))


def test_entry_points_are_declared_bound_and_exported():
    from modules import _native as N
    from test_host import header_symbols
    for s in ("abcd_chain_workspace_bytes", "abcd_chain_plan", "abcd_chain_posterior"):
        assert s in header_symbols() and s in N.EXPORTED and hasattr(N.lib(), s), s
    assert N.lib().abcd_dispatch_count(15) == -1 and N.lib().abcd_dispatch_count(17) == -1   # no new id
    assert N.library_hash() == N.source_hash()
    ws = N.lib().abcd_chain_workspace_bytes
    assert ws(100, 3, 0, 15) == 0 and ws(100, 3, 1025, 15) == 0 and ws(100, 3, 1024, 15) > 0
    assert ws(-1, 3, 4, 15) == 0 and ws(100, -1, 4, 15) == 0
    assert ws(1 << 24, 3, 128, 15) == 0 and ws((1 << 24) - 1, 3, 128, 1) > 0          # N * K >= 2^31
    assert ws(0, 0, 4, 15) > 0
    full, vit = ws(20000, 100, 128, 15), ws(20000, 100, 128, C.WANT_PATH)
    assert vit < full and vit >= 20000 * 128 * 2 and vit < 20000 * 128 * 4             # back-pointers, no stored alphas
    assert ws(20000, 100, 128, C.WANT_EVIDENCE) < 20000 * 4                            # the offsets only
    assert full >= 2 * 20000 * 128 * 4 + 100 * 128 * 128 * 8
    res, wg = ctypes.c_int(-1), ctypes.c_int(-1)
    plan = N.lib().abcd_chain_plan
    assert plan(128, 100, res, wg) == 0 and res.value == 1 and wg.value == 100
    assert plan(1024, 100, res, wg) == 0 and res.value == 0 and 1 <= wg.value <= 100
    assert plan(1024, 100, None, None) == 0
    assert plan(0, 1, res, wg) == N.ABCD_EINVAL and plan(1025, 1, res, wg) == N.ABCD_EINVAL
    assert plan(4, -1, res, wg) == N.ABCD_EINVAL
    assert C.plan(64, 1 << 20)[1] == C.plan(64, 1 << 21)[1]                            # capped
    assert 128 < C.first_streaming_k() <= 1024


def test_chain_posterior_rejects_bad_arguments_on_the_host():
    """ABCD_EINVAL is decided before any launch: no device is needed and the
    (fake, never dereferenced) pointers are not touched."""
    from modules import _native as N
    lib = N.lib()
    n, K, S = 6, 4, 3
    so = torch.tensor([0, 2, 2, 6], dtype=torch.int64)
    nbytes = lib.abcd_chain_workspace_bytes(n, S, K, 15)
    fake = N.c_void_p(4096)

    def call(score=fake, lds=K, n=n, K=K, so=so, S=S, lt=fake, ldt=K, li=fake, ev=fake, gamma=fake, ldg=K, path=fake,
             ps=fake, tc=fake, ic=fake, ws=fake, nb=nbytes):
        return lib.abcd_chain_posterior(score, lds, n, K, None if so is None else so.data_ptr(), S, lt, ldt, li, ev,
                                        gamma, ldg, path, ps, tc, ic, ws, nb, None)

    E = N.ABCD_EINVAL
    none = dict(ev=None, gamma=None, path=None, ps=None, tc=None, ic=None)
    assert call(K=0) == E and call(K=1025, lds=1025, ldt=1025, ldg=1025, nb=1 << 40) == E
    assert call(n=-1) == E and call(S=-1) == E
    big = torch.tensor([0, 1 << 24], dtype=torch.int64)
    assert call(n=1 << 24, K=128, lds=128, ldt=128, ldg=128, so=big, S=1, nb=1 << 50) == E       # N * K >= 2^31
    assert call(so=None) == E
    assert call(so=torch.tensor([0, 3, 2, 6], dtype=torch.int64)) == E                             # decreasing
    assert call(so=torch.tensor([1, 2, 2, 6], dtype=torch.int64)) == E                             # seq_off[0] != 0
    assert call(so=torch.tensor([0, 2, 2, 5], dtype=torch.int64)) == E                             # seq_off[S] != N
    assert call(lds=K - 1) == E and call(ldt=K - 1) == E and call(ldg=K - 1) == E                  # a stride below K
    assert call(score=None) == E and call(lt=None) == E and call(li=None) == E
    assert call(score=None, **dict(none, ps=fake)) == E                                            # one output is enough
    assert call(ws=None) == E and call(nb=nbytes - 1) == E and call(nb=0) == E
    # with every output NULL a valid call does nothing and needs no device, nor any input
    assert call(**none) == 0 and call(score=None, lt=None, li=None, **none) == 0
    assert call(ldg=0, **none) == 0
    assert call(n=0, so=torch.zeros(1, dtype=torch.int64), S=0, **none) == 0


def test_op_is_registered_with_a_fake_implementation():
    from modules import ops
    from modules.sequence import TransitionModel
    assert "chain_posterior" in ops.OPS and hasattr(torch.ops.abcd, "chain_posterior")
    assert set(ops.registered()) == set(ops.OPS)
    schema = str(torch.ops.abcd.chain_posterior.default._schema)
    assert schema.startswith("abcd::chain_posterior(Tensor score, Tensor seq_off, Tensor log_trans, Tensor log_init, "
                             "SymInt want) -> Tensor[]"), schema
    m = dict(device="meta")
    so = torch.tensor([0, 2, 2, 7])
    out = ops._chain_posterior_fake(torch.empty(7, 5, **m), so, torch.empty(5, 5, **m), torch.empty(5, **m), 15)
    ev, gamma, path, ps, tc, ic = out
    assert ev.shape == ps.shape == (3,) and ev.dtype == ps.dtype == torch.float64
    assert gamma.shape == (7, 5) and gamma.dtype == torch.float32 and path.shape == (7,) and path.dtype == torch.int32
    assert tc.shape == (5, 5) and ic.shape == (5,) and tc.dtype == ic.dtype == torch.float64
    assert all(t.device.type == "meta" for t in out)
    ev, gamma, path, ps, tc, ic = ops._chain_posterior_fake(torch.empty(7, 5, **m), so, torch.empty(5, 5, **m),
                                                            torch.empty(5, **m), ops.CHAIN_PATH)
    assert ev.numel() == gamma.numel() == tc.numel() == ic.numel() == 0 and path.shape == (7,) and ps.shape == (3,)
    assert (ops.CHAIN_EVIDENCE, ops.CHAIN_GAMMA, ops.CHAIN_PATH, ops.CHAIN_COUNTS) == (1, 2, 4, 8)
    assert ops.chain_plan(128, 7) == (True, 7) and ops.chain_plan(1024, 7)[0] is False
    # no CPU fallback anywhere
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.chain_posterior(torch.zeros(7, 5), so, torch.zeros(5, 5), torch.zeros(5), 15)
    model = TransitionModel(5)
    assert model.log_trans.shape == (5, 5) and model.log_init.shape == (5,) and "log_trans" in dict(model.named_buffers())
    assert torch.allclose(model.log_trans.exp().sum(1), torch.ones(5))
    with pytest.raises(RuntimeError, match="GPU only"):
        model.posterior(torch.zeros(7, 5), so)
    with pytest.raises(RuntimeError, match="GPU only"):
        model.viterbi(torch.zeros(7, 5), so)
    with pytest.raises(RuntimeError, match="GPU only"):
        model.fit(torch.zeros(7, 5), so, n_iter=1)
    cf = TransitionModel.from_log_weight(torch.tensor([0.5, -1.0, 2.0]))
    want = torch.log_softmax(torch.tensor([0.5, -1.0, 2.0], dtype=torch.float64), 0).float()
    assert torch.equal(cf.log_init, want) and all(torch.equal(cf.log_trans[i], want) for i in range(3))
    # chain_scores is plain torch: float64 differences, each row's maximum taken off
    em = torch.tensor([[5e4 + 1.0, 5e4 + 0.25, float("nan")], [float("inf"), float("nan"), float("nan")]])
    score, off = ops.chain_scores(em, None, torch.tensor([0.0, 0.5, 0.0]))
    assert score.dtype == torch.float32 and off.dtype == torch.float64
    assert score[0].tolist() == [-1.25, 0.0, -float("inf")] and off[0] == -5e4 - 0.25 + 0.5
    assert (score[1] == -float("inf")).all() and off[1] == 0


def test_split_sequences():
    from modules.sequence import split_sequences
    ann = pd.read_csv(ANN)
    n = len(ann)
    order, off = split_sequences(ann)
    assert ann["input_path"].nunique() == 1 and off.tolist() == [0, n]                # one file, one sequence
    assert sorted(order.tolist()) == list(range(n)) and (np.diff(ann["onset"].to_numpy()[order]) >= 0).all()
    sh = ann.sample(frac=1.0, random_state=3).reset_index(drop=True)                 # a shuffled table: onset order
    o2, f2 = split_sequences(sh)
    assert f2.tolist() == [0, n] and sh["onset"].to_numpy()[o2].tolist() == sorted(ann["onset"].tolist())
    # the toy segments touch one another: open a 0.1 s gap before row 3 and a 0.2 s gap before row 6
    gp = ann.copy()
    gp.loc[3, "onset"] += 0.1
    gp.loc[6, "onset"] += 0.2
    assert split_sequences(gp, max_gap=0.25)[1].tolist() == [0, n]                    # no gap above max_gap: no split
    o3, f3 = split_sequences(gp, max_gap=0.15)                                        # below the largest gap
    assert o3.tolist() == order.tolist() and f3.tolist() == [0, 6, n]
    assert split_sequences(gp, max_gap=0.05)[1].tolist() == [0, 3, 6, n]
    assert split_sequences(gp, max_gap=0.0)[1].tolist() == [0, 3, 6, n]               # touching segments stay together
    # a second column splits it; the groups come in sorted key order, each in onset order
    assert ann["speaker"].nunique() > 1
    o4, f4 = split_sequences(ann, by=("input_path", "speaker"))
    assert len(f4) - 1 == ann["speaker"].nunique() and f4[-1] == n and sorted(o4.tolist()) == list(range(n))
    spk = ann["speaker"].to_numpy()[o4]
    for s in range(len(f4) - 1):
        part = slice(f4[s], f4[s + 1])
        assert len(set(spk[part])) == 1 and (np.diff(ann["onset"].to_numpy()[o4][part]) >= 0).all()
    assert [str(spk[f4[s]]) for s in range(len(f4) - 1)] == sorted(str(v) for v in ann["speaker"].unique())
    e_o, e_f = split_sequences(ann.iloc[:0])
    assert e_o.tolist() == [] and e_f.tolist() == [0]


def test_sequence_cli_arguments():
    import classify
    import sequence
    a = sequence.get_parameters(["ckpt.pt", "root", "ann.csv", "1.0"])
    assert (a.model_path, a.input_root, a.annotation_file, a.data_normalizer) == ("ckpt.pt", "root", "ann.csv", 1.0)
    assert a.em_iterations == 10 and a.pseudo_count is None and a.max_gap is None and a.transitions is None
    assert a.sequence_columns == ["input_path"] and a.prior == "dirichlet" and a.save_path is None
    a = sequence.get_parameters(["c", "r", "a", "2.5", "--em_iterations", "0", "--pseudo_count", "0.5", "--max_gap",
                                 "1.5", "--sequence_columns", "input_path", "speaker", "--prior", "uniform",
                                 "--transitions", "t.csv", "-b", "4", "-S", "out"])
    assert (a.em_iterations, a.pseudo_count, a.max_gap, a.sequence_columns, a.prior, a.transitions, a.batch_size,
            a.save_path) == (0, 0.5, 1.5, ["input_path", "speaker"], "uniform", "t.csv", 4, "out")
    for bad in (["--prior", "flat"], ["--em_iterations", "-1"], ["--pseudo_count", "-1"], ["--max_gap", "-2"],
                ["--entire_data_size", "0"]):
        with pytest.raises(SystemExit):
            sequence.get_parameters(["c", "r", "a", "1"] + bad)
    # the same positional and STFT arguments as classify.py
    c = vars(classify.get_parameters(["c", "r", "a", "1"]))
    s = vars(sequence.get_parameters(["c", "r", "a", "1"]))
    shared = set(c) - {"matrix"}
    assert shared <= set(s) and all(s[k] == c[k] for k in shared)
    assert issubclass(sequence.Sequencer, classify.Classifier)
    assert sequence.COLUMNS == ("data_ix", "sequence_ix", "position", "decoder_category_ix", "smoothed_category_ix",
                                "smoothed_category_prob", "viterbi_category_ix", "changed")
    assert sequence.TRANSITION_COLUMNS == ("from_ix", "to_ix", "probability", "expected_count")
    assert sequence.SEQUENCE_COLUMNS == ("sequence_ix", "length", "log_evidence", "context_free_log_evidence")
