"""Time-warped scoring without a GPU: the float64 reference of
``warp_cases.py`` against brute-force enumeration, its special cases and
inequalities, ``modules/alignment.py`` on hand-written paths, the operators'
registration and argument checks, and ``align.py``'s arguments and table."""
import math

import numpy as np
import pytest
import torch

import pairwise_cases as PW
import warp_cases as W

NINF = -math.inf


# ----------------------------------------------------------------------------
# the reference
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("marginal", (False, True))
@pytest.mark.parametrize("band", (-1, 0, 1, 2))
def test_reference_equals_brute_force(band, marginal):
    rng = np.random.default_rng(17 + band)
    worst = 0.0
    for n, S_ in ((7, 9), (5, 3), (1, 4), (6, 1), (7, 14)):
        c = rng.normal(size=(n, S_)) * 3.0 + 10.0
        if S_ > 3 and n > 2:
            c[2, 3] = np.nan  # an excluded cell
        for moves in list(W.MOVES.values()) + [(math.log(0.7), NINF, math.log(0.3))]:
            a = float(W.dp(c[None], np.array([n]), moves, band, marginal)["value"][0])
            b = W.brute_force(c, n, moves, band, marginal)
            if np.isinf(a) or np.isinf(b):
                assert a == b, (n, S_, moves)
            else:
                worst = max(worst, abs(a - b))
    print(f"band {band} marginal {marginal}: worst |recurrence - enumeration| {worst:.2e}")
    assert worst <= 1e-12


def test_viterbi_path_is_the_enumerations_best_and_ties_go_low():
    rng = np.random.default_rng(5)
    c = rng.normal(size=(6, 8)) + 4.0
    moves = W.MOVES["default"]
    r = W.dp(c[None], np.array([6]), moves)
    path = W.backtrack(r["back"][0], r["end"][0], 6)
    cost, mcost = W.path_cost(c, path, moves)
    assert abs(cost + mcost - r["value"][0]) <= 1e-12 and path[0] == 0
    # all costs equal and all moves alike: the lowest move (stay) and the lowest final state win
    flat = W.dp(np.ones((1, 4, 6)), np.array([4]), (0.0, 0.0, 0.0))
    assert flat["end"][0] == 0 and W.backtrack(flat["back"][0], 0, 4).tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("shape,F,P", (("ties", 65, 17), ("b33t9", 1, 33), ("b40t37", 129, 1)))
def test_identity_moves_reduce_to_pairwise_reference(shape, F, P):
    c = PW.abi_inputs(shape, F, P)  # T_proto = T
    for marginal in (False, True):
        r = W.warp_reference(c["batch_sizes"], c["gt"], c["mu"], c["lv"], c["o"], c["y"], W.MOVES["identity"],
                             marginal=marginal)
        want = c["ref"]["em"] + c["ref"]["off"]
        assert np.abs(r["value"] - want).max() <= 1e-11 * np.abs(want).max()
    assert all(p.tolist() == list(range(len(p))) for p in r["paths"].values())
    assert np.abs(r["em"] - c["ref"]["em"]).max() <= 1e-11 * np.abs(c["ref"]["em"]).max()
    assert np.abs(r["off"] - c["ref"]["off"]).max() <= 1e-11 * c["ref"]["off"].max()
    assert (r["move"] == 0).all()
    # the unit is pairwise_cases' A plus the |BCE| terms
    assert np.abs(r["A"] - (c["ref"]["A"] + c["ref"]["off"])).max() <= 1e-11 * r["A"].max()


@pytest.mark.parametrize("case", [c for c in W.ABI_CASES if c[0] in ("ties", "b33t9")], ids=W.case_id)
def test_marginal_below_viterbi_below_identity_path(case):
    shape, F, P, ld, kind, band, mname = case
    c = W.abi_inputs(shape, F, P, kind)
    vit = W.abi_reference(shape, F, P, kind, band, mname, False)
    mar = W.abi_reference(shape, F, P, kind, band, mname, True)
    fin = np.isfinite(vit["value"])
    assert np.array_equal(fin, np.isfinite(mar["value"]))
    assert (mar["value"][fin] <= vit["value"][fin] + 1e-9).all()
    moves = W.MOVES[mname]
    if c["S"] >= c["T"] and moves[1] > NINF:  # the identity path exists: the best path costs no more
        for (b, p), path in vit["paths"].items():
            n = len(path)
            ident = sum(vit["c"][b, p, t, t] for t in range(n)) - (n - 1) * moves[1]
            assert vit["value"][b, p] <= ident + 1e-9
    for (b, p), path in vit["paths"].items():
        cost, mcost = W.path_cost(vit["c"][b, p], path, moves)
        assert abs(cost + mcost - vit["value"][b, p]) <= 1e-9 * vit["A"][b, p]
        assert abs(vit["em"][b, p] + vit["off"][b, p] + vit["move"][b, p] - vit["value"][b, p]) <= 1e-9 * vit["A"][b, p]


def test_unreachable_pairs_are_inf():
    c = W.abi_inputs("b33t9", 129, 1, "one")  # one state, stay disabled: only one-frame segments align
    r = W.abi_reference("b33t9", 129, 1, "one", -1, "stepskip", False)
    lens = r["lengths"]
    assert np.array_equal(np.isposinf(r["value"][:, 0]), lens > 1) and (lens > 1).any() and (lens == 1).any()
    assert c["S"] == 1


def test_planted_alignments_are_the_references_optimum():
    for name, plant in W.PLANTS.items():
        c = W.planted(name)
        r = W.warp_reference(c["batch_sizes"], c["gt"], c["mu"], c["lv"], c["o"], c["y"], W.MOVES["default"])
        assert r["paths"][(0, W.PLANT_CAT)].tolist() == plant
        v = r["value"][0]
        assert int(v.argmin()) == W.PLANT_CAT and np.sort(v)[1] - v[W.PLANT_CAT] > 400.0


def test_cases_cover_the_product():
    cases = W.ABI_CASES
    assert {c[0] for c in cases} >= {"b1t1", "ties", "b33t9", "b40t37"}
    assert {c[1] for c in cases} == {1, 65, 129} and {c[2] for c in cases} >= {1, 17, 33}
    assert {c[3] for c in cases} == {0, 144} and {c[4] for c in cases} == {"one", "short", "long", "double"}
    assert {c[5] for c in cases} >= {-1, 0, 3} and {c[6] for c in cases} == set(W.MOVES)
    long = [c for c in cases if c[0] == "b40t37"]
    assert {c[4] for c in long} == {"one", "short", "long", "double"} and {c[5] for c in long} == {-1, 0, 3}
    assert [W.proto_steps(k, 37) for k in ("one", "short", "long", "double")] == [1, 35, 40, 75]
    assert W.proto_steps("short", 1) == 1
    # a band edge on a super-block boundary at the start of a frame block, on the shape that has 128 frames and more
    edge = [c for c in cases if c[0] == "b3t170" and c[5] >= 0 and any((t0 - c[5]) % 128 == 0 and t0 > c[5]
                                                                        for t0 in range(128, 170, 32))]
    assert {c[5] for c in edge} == {0, 32}


# ----------------------------------------------------------------------------
# modules/alignment.py
# ----------------------------------------------------------------------------
def _pack(paths):
    """hand-written per-segment paths (longest first) -> (packed states, batch_sizes)"""
    T = len(paths[0])
    bs = [sum(len(p) > t for p in paths) for t in range(T)]
    return torch.tensor([p[t] for t in range(T) for p in paths if len(p) > t]), torch.tensor(bs)


def test_summarize_paths_and_fit_moves():
    from modules import alignment as A
    paths = [[0, 0, 1, 3, 3, 4], [0, 2, 4, 6], [-1, -1, -1], [0]]
    states, bs = _pack(paths)
    s = A.summarize_paths(states, bs)
    assert s["end_state"].tolist() == [4, 6, -1, 0] and s["length"].tolist() == [6, 4, 3, 1]
    assert s["n_stay"].tolist() == [2, 0, 0, 0] and s["n_skip"].tolist() == [1, 3, 0, 0]
    assert s["tempo"].tolist() == [5 / 6, 7 / 4, 0.0, 1.0]
    # counts: stay 2, step 2, skip 4 (the segment without a path counts nothing)
    lm = A.fit_moves(states, bs, smoothing=1.0)
    assert np.allclose(np.exp(lm), np.array([3, 3, 5]) / 11.0) and abs(sum(np.exp(lm)) - 1.0) < 1e-12
    lm0 = A.fit_moves(states, bs, smoothing=0.0)
    assert np.allclose(np.exp(lm0), np.array([2, 2, 4]) / 8.0)
    kept = A.fit_moves(states, bs, smoothing=1.0, log_moves=(NINF, 0.0, 0.0))
    assert kept[0] == NINF and np.allclose(np.exp(kept[1:]), np.array([3, 5]) / 8.0)
    with pytest.raises(ValueError):
        A.fit_moves(torch.tensor([0]), torch.tensor([1]), smoothing=0.0)
    with pytest.raises(ValueError):
        A.summarize_paths(states[:-1], bs)
    assert A.moves_from_probabilities([1, 3, 1]) == pytest.approx(W.MOVES["default"])
    assert A.moves_from_probabilities([0, 2, 0]) == (NINF, 0.0, NINF)
    for bad in ([0, 0, 0], [1, -1, 1], [1, 1], [float("nan"), 1, 1]):
        with pytest.raises(ValueError):
            A.moves_from_probabilities(bad)


# ----------------------------------------------------------------------------
# the operators and the tool
# ----------------------------------------------------------------------------
def test_ops_registered_and_refuse_cpu_tensors():
    from modules import ops
    for name in ("warp_nll", "warp_path"):
        assert name in ops.OPS and hasattr(torch.ops.abcd, name)
    assert set(ops.registered()) == set(ops.OPS)
    assert ops.DEFAULT_LOG_MOVES == pytest.approx(W.MOVES["default"]) and ops.IDENTITY_LOG_MOVES == W.MOVES["identity"]
    c = W.planted("mixed")
    args = (c["gt"], torch.from_numpy(c["batch_sizes"]), c["y"], c["mu"].reshape(-1, c["F"]),
            c["lv"].reshape(-1, c["F"]), c["o"].reshape(-1))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        torch.ops.abcd.warp_nll(*args, list(ops.DEFAULT_LOG_MOVES), -1, False, c["P"], c["F"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        torch.ops.abcd.warp_path(*args, list(ops.DEFAULT_LOG_MOVES), -1, torch.zeros(1, dtype=torch.int32), c["P"],
                                 c["F"])


def test_fakes_give_the_output_shapes():
    from modules import ops
    # B is batch_sizes[0], a value: the registered fake implementations are called on meta tensors with real batch_sizes
    bs, m = torch.tensor([3, 2, 2, 1]), dict(device="meta")
    gt, y = torch.empty(8, 5, **m), torch.empty(8, **m)
    mu, lv, o = torch.empty(6 * 4, 5, **m), torch.empty(6 * 4, 5, **m), torch.empty(6 * 4, **m)
    w = ops._warp_nll_fake(gt, bs, y, mu, lv, o, list(ops.DEFAULT_LOG_MOVES), -1, False, 4, 5)
    assert tuple(w.shape) == (3, 4) and w.dtype == torch.float32 and w.device.type == "meta"
    st, pe, po, pm = ops._warp_path_fake(gt, bs, y, mu, lv, o, list(ops.DEFAULT_LOG_MOVES), 2,
                                         torch.empty(3, dtype=torch.int32, **m), 4, 5)
    assert tuple(st.shape) == (8,) and st.dtype == torch.int32
    assert tuple(pe.shape) == tuple(po.shape) == tuple(pm.shape) == (3,) and pe.dtype == torch.float32
    schema = str(torch.ops.abcd.warp_nll.default._schema)
    assert schema.startswith("abcd::warp_nll(Tensor gt, Tensor batch_sizes, Tensor gt_offset, Tensor proto_mu, "
                             "Tensor proto_lv, Tensor proto_offset_logits, float[] log_moves, SymInt band, "
                             "bool marginal, SymInt P, SymInt F) -> Tensor"), schema


def test_workspace_queries_and_limits():
    from modules import _native as N
    lib = N.lib()
    assert lib.abcd_warp_nll_workspace_bytes(200, 512, 128, 300) >= 201 * 4
    assert lib.abcd_warp_path_workspace_bytes(200, 512, 300) >= 512 * 200 * 300 * 5
    assert lib.abcd_warp_path_workspace_bytes(10, 2, 16383) >= 2 * 10 * 19 * 5  # a path reaches 2 T - 1 states
    assert lib.abcd_warp_path_workspace_bytes(10, 2, 16383) < 2 * 10 * 16383
    for bad in ((0, 1, 1, 1), (4097, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0), (1, 1, 1, 16384),
                (1, 1 << 16, 1 << 15, 1)):
        assert lib.abcd_warp_nll_workspace_bytes(*bad) == 0, bad
    assert lib.abcd_warp_path_workspace_bytes(4097, 1, 1) == 0 and lib.abcd_warp_path_workspace_bytes(1, 1, 16384) == 0


def test_align_cli_arguments_and_header():
    import align
    import classify
    base = ["c", "r", "t", "1"]
    a = align.get_parameters(base)
    assert (a.moves, a.band, a.marginal, a.proto_factor, a.fit_moves, a.paths) == ([0.2, 0.6, 0.2], None, False, 1.5,
                                                                                  0, None)
    assert (a.prior, a.entire_data_size, a.batch_size, a.annotation_file) == ("dirichlet", None, 1, "t")
    a = align.get_parameters(base + ["--moves", "0", "1", "0", "--band", "4", "--marginal", "--proto_factor", "2",
                                     "--fit_moves", "3", "--paths", "p.csv", "-b", "8"])
    assert (a.moves, a.band, a.marginal, a.proto_factor, a.fit_moves, a.paths, a.batch_size) == \
        ([0.0, 1.0, 0.0], 4, True, 2.0, 3, "p.csv", 8)
    for bad in (["--moves", "0", "0", "0"], ["--moves", "1", "-1", "1"], ["--moves", "1", "1"], ["--band", "-1"],
                ["--proto_factor", "0"], ["--fit_moves", "-1"], ["--prior", "flat"], ["--entire_data_size", "0"]):
        with pytest.raises(SystemExit):
            align.get_parameters(base + bad)
    # classify.py's identifying columns, then the warped ones
    assert align.COLUMNS[:4] == classify.COLUMNS[:4] == ("data_ix", "length", "category_ix", "category_prob")
    assert align.COLUMNS[4:] == ("warp_category_ix", "warp_nll", "warp_log_evidence", "warp_best_prob", "end_state",
                                 "tempo", "n_stay", "n_skip")
    assert tuple(n for n, _ in align.TABLE) == align.COLUMNS[1:]
    assert align.PATH_COLUMNS == ("data_ix",) + tuple(n for n, _ in align.PATHS)
    assert issubclass(align.Aligner, classify.Classifier)
