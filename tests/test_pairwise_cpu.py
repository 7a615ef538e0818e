"""Pairwise scoring, checked on the CPU: the float64 references of
``pairwise_cases.py`` (every segment against every prototype, the categorical
posterior) against ``score_cases.segment_reference`` on one prototype at a time
and against the variational bound they are meant to attain; the new entry
points' surface (header, binding, ids, host-side argument checks, custom ops,
methods); ``classify.py``'s arguments and the generalised table writer with a
stub batch function."""
import os

import numpy as np
import pandas as pd
import pytest
import torch

import pairwise_cases as PW
import score_cases as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOY = os.path.join(GOLDEN, "toy_data")
ANN = os.path.join(TOY, "annotation_20170806-080002_89.2-94.22.csv")


@pytest.mark.parametrize("shape", list(PW.ABI_SHAPES))
def test_pairwise_reference_is_segment_reference_per_prototype(shape):
    for F, P in ((1, 17), (65, 33), (129, 1), (129, 17)):
        c = PW.abi_inputs(shape, F, P)
        ref, bs = c["ref"], c["batch_sizes"]
        assert ref["em"].shape == ref["A"].shape == ref["off"].shape == (c["B"], P)
        assert ref["lengths"].tolist() == list(c["lengths"])
        for p in range(P):
            mu, lv, o = PW.expand_prototype(bs, p, c["mu"], c["lv"], c["o"])
            one = S.segment_reference(bs, c["gt"], mu, lv, o, c["y"])
            assert np.abs(ref["em"][:, p] - one["em"]).max() <= 1e-12 * one["A"].max()
            assert np.abs(ref["A"][:, p] - one["A"]).max() <= 1e-12 * one["A"].max()
            assert np.abs(ref["off"][:, p] - one["off"]).max() <= 1e-12 * max(one["off"].max(), 1.0)
        assert (ref["A"] >= np.abs(ref["em"])).all() and (ref["off"] >= 0).all()
    own = PW.ABI_SHAPES["b40t37"]
    assert len(own) == 40 and own == sorted(own, reverse=True) and own[0] > 32 and own[32] <= 16
    # a segment is drawn around its own prototype: that column is its smallest NLL wherever there is a choice
    c = PW.abi_inputs("b33t9", 129, 33)
    assert (c["ref"]["em"].argmin(1) == c["own"].numpy()).all()


def test_posterior_reference_attains_the_variational_bound():
    """F(q) = sum_k q_k (nll_k + log q_k - lw_k) >= -log_evidence for every q on
    the simplex, with equality at the responsibilities."""
    g = np.random.default_rng(5)
    for B, P in ((5, 16), (33, 65), (1, 130)):
        c = PW.posterior_inputs(B, P)
        ref = c["ref"]
        nll = c["em"].double().numpy() + c["off"].double().numpy()
        lw = c["lw"].double().numpy()

        def free(q):
            with np.errstate(divide="ignore", invalid="ignore"):
                return np.where(q > 0, q * (nll + np.log(q) - lw[None]), 0.0).sum(1)
        assert np.abs(free(ref["resp"]) + ref["log_evidence"]).max() <= 1e-9 * np.abs(ref["log_evidence"]).max()
        assert np.abs(ref["resp"].sum(1) - 1.0).max() <= 1e-12
        for _ in range(20):
            q = g.dirichlet(np.full(P, 0.3), size=B)
            assert (free(q) >= -ref["log_evidence"] - 1e-9 * np.abs(ref["log_evidence"])).all()
        assert (ref["best_prob"] == ref["resp"].max(1)).all()


def test_posterior_cases_decide_their_winner():
    for B in PW.POST_B:
        for P in PW.POST_P:
            ref = PW.posterior_inputs(B, P)["ref"]
            assert (PW.top_two_gap(ref["s"]) >= 0.5).all(), (B, P)
            assert ref["best"].shape == (B,) and (ref["best"] >= 0).all()
    # exclusion rules of the reference
    em = torch.tensor([[1.0, float("nan"), 2.0, float("inf")], [float("nan")] * 4, [3.0, 3.0, 5.0, 3.0]])
    lw = torch.tensor([0.0, 0.0, float("-inf"), 0.0])
    r = PW.posterior_reference(em, None, lw)
    assert r["best"].tolist() == [0, -1, 0] and r["resp"][0].tolist() == [1.0, 0.0, 0.0, 0.0]
    assert r["log_evidence"][0] == -1.0 and r["log_evidence"][1] == -np.inf and r["best_prob"][1] == 0.0
    assert np.allclose(r["resp"][2], [1 / 3, 1 / 3, 0.0, 1 / 3]) and (r["resp"][1] == 0).all()


def _packed(N, bs, L, B, F, T=None):
    return N.Packed(None, bs.data_ptr(), int(bs.numel()) if T is None else T, L, B, F)


def test_new_entry_points_are_declared_bound_and_exported():
    from modules import _native as N
    from test_host import header_symbols
    for s in ("abcd_pairwise_nll_workspace_bytes", "abcd_pairwise_nll", "abcd_pair_posterior"):
        assert s in header_symbols() and s in N.EXPORTED and hasattr(N.lib(), s), s
    assert (N.PAIR_NLL, N.PAIR_POST) == (13, 14)
    assert N.lib().abcd_dispatch_count(13) >= 0 and N.lib().abcd_dispatch_count(14) >= 0  # ids inside TK_N
    assert N.lib().abcd_dispatch_count(15) == -1
    ws = N.lib().abcd_pairwise_nll_workspace_bytes
    assert ws(200, 512, 128) >= 201 * 4 + 2 * 13 * 512 * 128 * 8  # offsets and fp64 partials of 13 slices, twice
    assert ws(0, 4, 4) == 0 and ws(4, 0, 4) == 0 and ws(4, 4, 0) == 0 and ws(1 << 20, 4, 4) == 0
    assert ws(16383, 1, 1) > 0 and ws(16384, 1, 1) == 0
    assert ws(4, 1 << 16, 1 << 15) == 0 and ws(4, 1 << 15, (1 << 16) - 1) > 0  # B * P >= 2^31


def test_pairwise_nll_rejects_bad_arguments_on_the_host():
    """ABCD_EINVAL is decided before any launch: no device is needed and the
    (fake, never dereferenced) pointers are not touched."""
    from modules import _native as N
    lib = N.lib()
    bs = torch.tensor([3, 2, 1], dtype=torch.int64)
    T, L, B, F, P = 3, 6, 3, 4, 5
    nbytes = lib.abcd_pairwise_nll_workspace_bytes(T, B, P)
    fake = N.c_void_p(4096)  # a non-NULL pointer: every case below is refused before it could be read

    def call(bs=bs, T=None, L=L, B=B, F=F, data=fake, y=fake, P=P, Tp=T, mu=fake, ldm=F, lv=fake, ldl=F, o=fake,
             em=fake, off=fake, ldp=P, ws=fake, nb=nbytes):
        pk = _packed(N, bs, L, B, F, T)
        pk.data = data
        return lib.abcd_pairwise_nll(pk, y, P, Tp, mu, ldm, lv, ldl, o, em, off, ldp, ws, nb, None)

    E = N.ABCD_EINVAL
    assert E == 1000
    assert call(bs=torch.tensor([2, 3, 1], dtype=torch.int64)) == E   # batch_sizes not non-increasing
    assert call(B=2) == E and call(L=7) == E                           # batch_sizes[0] != B, sum != L
    assert call(bs=torch.zeros(0, dtype=torch.int64), T=0) == E
    assert call(P=0) == E and call(P=-1) == E
    assert call(Tp=T - 1) == E                                         # a rectangle shorter than the batch
    assert call(ldm=F - 1) == E and call(ldl=F - 1) == E               # a stride below F
    assert call(ldp=P - 1) == E
    assert call(data=None) == E and call(mu=None) == E and call(lv=None) == E   # pair_em without its inputs
    assert call(y=None) == E and call(o=None) == E                     # pair_off without both of its inputs
    assert call(ws=None) == E and call(nb=nbytes - 1) == E and call(nb=0) == E
    long = torch.ones(16384, dtype=torch.int64)
    assert call(bs=long, L=16384, B=1, nb=1 << 40) == E               # T > 16383
    # with both outputs NULL a valid call does nothing and needs no device either
    assert call(em=None, off=None) == 0
    # the posterior's host checks
    post = lib.abcd_pair_posterior
    assert post(None, None, 4, 2, 4, None, fake, None, None, None, 0, None) == E
    assert post(fake, None, 3, 2, 4, None, fake, None, None, None, 0, None) == E   # ld_pair < P
    assert post(fake, None, 4, 0, 4, None, fake, None, None, None, 0, None) == E
    assert post(fake, None, 4, 2, 0, None, fake, None, None, None, 0, None) == E
    assert post(fake, None, (1 << 20) + 1, 2, (1 << 20) + 1, None, fake, None, None, None, 0, None) == E
    assert post(fake, None, 4, 2, 4, None, None, None, None, fake, 3, None) == E   # ld_resp < P
    assert post(fake, None, 4, 2, 4, None, None, None, None, None, 0, None) == 0   # nothing asked for


def test_ops_and_methods_exist():
    from modules import model as M, ops
    for name in ("pairwise_nll", "pair_posterior"):
        assert name in ops.OPS and hasattr(torch.ops.abcd, name)
    assert set(ops.registered()) == set(ops.OPS)
    schema = str(torch.ops.abcd.pairwise_nll.default._schema)
    assert schema.startswith("abcd::pairwise_nll(Tensor? gt, Tensor batch_sizes, Tensor? gt_offset, Tensor? proto_mu, "
                             "Tensor? proto_lv, Tensor? proto_offset_logits, SymInt P, SymInt F) -> Tensor[]"), schema
    schema = str(torch.ops.abcd.pair_posterior.default._schema)
    assert schema.startswith("abcd::pair_posterior(Tensor pair_em, Tensor? pair_off, Tensor? log_weight) -> Tensor[]"), \
        schema
    from torch._subclasses.fake_tensor import FakeTensorMode
    # B is batch_sizes[0], a value: the registered fake implementation is called on meta tensors with real batch_sizes
    m = dict(device="meta")
    em, off = ops._pairwise_nll_fake(torch.empty(6, 4, **m), torch.tensor([3, 2, 1]), torch.empty(6, **m),
                                     torch.empty(15, 4, **m), torch.empty(15, 4, **m), torch.empty(15, **m), 5, 4)
    assert em.shape == off.shape == (3, 5) and em.dtype == torch.float32 and em.device.type == "meta"
    with FakeTensorMode():
        ev, best, bp, resp = torch.ops.abcd.pair_posterior(torch.empty(3, 5), None, torch.empty(5))
        assert ev.shape == best.shape == bp.shape == (3,) and resp.shape == (3, 5) and best.dtype == torch.int32
    for f in (M.RNN_Variational_Decoder.prototypes, M.RNN_Variational_Decoder.score_against,
              M.ABCDSampler.expected_log_prior):
        assert callable(f)
    # no CPU fallback anywhere
    dec = M.RNN_Variational_Decoder(33, 32, 32, 32)
    with pytest.raises(RuntimeError, match="GPU only"):
        dec.prototypes(torch.zeros(4, 32), 3)
    protos = (torch.zeros(3, 4, 33), torch.zeros(3, 4, 33), torch.zeros(3, 4))
    with pytest.raises(RuntimeError, match="GPU only"):
        dec.score_against(protos, torch.tensor([2, 1]), torch.zeros(3, 33))
    with pytest.raises(RuntimeError, match="GPU only"):
        M.ABCDSampler(32, 32, 16, 32).expected_log_prior(100)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.pairwise_nll(torch.zeros(3, 33), torch.tensor([2, 1]), None, torch.zeros(8, 33), torch.zeros(8, 33), None,
                         4, 33)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.pair_posterior(torch.zeros(3, 5), None, None)


def test_classify_cli_arguments():
    import classify
    import score
    a = classify.get_parameters(["ckpt.pt", "root", "ann.csv", "1.0"])
    assert (a.model_path, a.input_root, a.annotation_file, a.data_normalizer) == ("ckpt.pt", "root", "ann.csv", 1.0)
    assert a.prior == "dirichlet" and a.entire_data_size is None and a.matrix is None
    assert a.batch_size == 1 and a.save_path is None and a.epsilon == 2 ** -15 and a.device == "cuda"
    a = classify.get_parameters(["c", "r", "a", "2.5", "--prior", "uniform", "--entire_data_size", "5000", "--matrix",
                                 "m.csv", "-b", "4", "-d", "cuda:1", "-S", "out.csv"])
    assert (a.prior, a.entire_data_size, a.matrix, a.batch_size, a.device, a.save_path) == \
        ("uniform", 5000.0, "m.csv", 4, "cuda:1", "out.csv")
    for bad in (["--prior", "flat"], ["--entire_data_size", "0"]):
        with pytest.raises(SystemExit):
            classify.get_parameters(["c", "r", "a", "1"] + bad)
    # the same positional and STFT arguments as score.py
    s = vars(score.get_parameters(["c", "r", "a", "1"]))
    c = vars(classify.get_parameters(["c", "r", "a", "1"]))
    shared = set(s) - {"mean", "sample", "samples", "seed"}
    assert shared <= set(c) and all(c[k] == s[k] for k in shared)
    assert classify.COLUMNS == ("data_ix",) + tuple(n for n, _ in classify.TABLE)
    assert classify.MATRIX_COLUMNS == ("data_ix",) + tuple(n for n, _ in classify.MATRIX)


def _toy_dataset():
    from modules import data_utils
    from modules.data_utils import Compose
    parser = data_utils.Data_Parser(TOY, ANN)
    fs = parser.get_sample_freq()
    tfm = Compose([data_utils.ToTensor(), data_utils.STFT(int(np.floor(0.008 * fs)), int(np.floor(0.004 * fs))),
                   data_utils.Transform(lambda x: (x + 2 ** -15).log() / 1.0)])
    return parser.get_data(transform=tfm)


def test_table_writer_with_classify_columns_and_stub(tmp_path):
    """score.score_table with classify.py's column lists and a batch function
    that returns known values: one row per segment mapped back to data_ix, the
    long table category-major within a batch, annotation columns appended to
    both, earlier outputs kept as .prev, nothing partial after a failure."""
    import classify
    import score
    ds = _toy_dataset()
    n, K = len(ds), 3

    def stub(packed, is_offset, speaker):
        seqs = torch.nn.utils.rnn.unpack_sequence(packed)
        B = len(seqs)
        lens = torch.tensor([s.shape[0] for s in seqs])
        first = torch.stack([s[0, 0] for s in seqs]).double()
        grid = first[:, None] + torch.arange(K)[None, :]                      # B x K
        return {"length": lens, "category_ix": lens % K, "category_prob": first * 0 + 0.5,
                "decoder_category_ix": (lens + 1) % K, "decoder_category_prob": first * 0 + 0.25,
                "log_evidence": -first, "agree": (lens % K) == ((lens + 1) % K),
                "long": {"row": torch.arange(B).repeat(K), "category_ix": torch.arange(K).repeat_interleave(B),
                         "emission_nll": grid.t().reshape(-1), "end_prediction_loss": grid.t().reshape(-1) * 2,
                         "log_weight": torch.arange(K).repeat_interleave(B).double() * -1.0,
                         "responsibility": torch.full((B * K,), 1.0 / K)}}

    out = os.path.join(str(tmp_path), "sub", "classified.csv")
    mat = os.path.join(str(tmp_path), "sub", "matrix.csv")
    os.makedirs(os.path.dirname(out))
    done = []
    kw = dict(columns=classify.TABLE, long_path=mat, long_columns=classify.MATRIX)
    assert score.score_table(stub, ds, out, batch_size=3, finish=lambda: done.append(1), **kw) == n
    assert done == [1]
    df, lt = pd.read_csv(out), pd.read_csv(mat)
    ann_cols = ["onset", "offset", "input_path", "data_type", "speaker", "label"]
    assert list(df.columns) == list(classify.COLUMNS) + ann_cols
    assert list(lt.columns) == list(classify.MATRIX_COLUMNS) + ann_cols
    assert sorted(df["data_ix"].tolist()) == list(range(n)) and len(df) == n and len(lt) == n * K
    ann = pd.read_csv(ANN)
    for _, row in df.iterrows():
        ix = int(row["data_ix"])
        seq, _ = ds[ix]
        assert row["length"] == seq.shape[0] and row["category_ix"] == seq.shape[0] % K and row["agree"] == 0
        assert row["log_evidence"] == pytest.approx(-float(seq[0, 0]), rel=1e-12)
        assert row["label"] == ann["label"][ix]
    # the long table: per batch, category 0 of all of its segments, then category 1, ...
    from modules import data_utils
    want_ix, want_k = [], []
    for _, _, _, ixs in data_utils.DataLoader(ds, batch_size=3, shuffle=False):
        want_ix += [int(i) for i in ixs] * K
        want_k += [k for k in range(K) for _ in ixs]
    assert lt["data_ix"].tolist() == want_ix and lt["category_ix"].tolist() == want_k
    assert df["data_ix"].tolist() == [i for j, i in enumerate(want_ix) if want_k[j] == 0]
    for _, row in lt.iterrows():
        seq, _ = ds[int(row["data_ix"])]
        assert row["emission_nll"] == pytest.approx(float(seq[0, 0]) + row["category_ix"], rel=1e-12)
        assert row["log_weight"] == -row["category_ix"] and row["label"] == ann["label"][int(row["data_ix"])]
    # a rerun keeps both earlier tables; a failing run leaves nothing partial
    score.score_table(stub, ds, out, batch_size=8, **kw)
    names = ["classified.csv", "classified.csv.prev", "matrix.csv", "matrix.csv.prev"]
    assert sorted(os.listdir(os.path.dirname(out))) == names

    def failing(packed, is_offset, speaker):
        raise RuntimeError("device lost")
    with pytest.raises(RuntimeError):
        score.score_table(failing, ds, out, batch_size=3, **kw)
    assert sorted(os.listdir(os.path.dirname(out))) == names and len(pd.read_csv(out)) == n
