"""Per-segment scoring, checked on the CPU: the float64 reference of
``score_cases.py`` (segmented sums over the packed layout) against a
per-sequence loop on the padded form and against the oracle's batch scalars on
the ``small_lstm_*`` fixtures; the new entry points' surface (header, binding,
custom ops, methods); ``score.py``'s arguments and its table writer with a
stub scorer."""
import os

import numpy as np
import pandas as pd
import pytest
import torch

import score_cases as S
from golden_io import SMALL

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOY = os.path.join(GOLDEN, "toy_data")
ANN = os.path.join(TOY, "annotation_20170806-080002_89.2-94.22.csv")
SMALL_LSTM = [n for n in SMALL if n.startswith("lstm_")]


@pytest.mark.parametrize("shape", list(S.ABI_SHAPES))
def test_segmented_sums_match_padded_loop(shape):
    for F in S.ABI_F:
        c = S.abi_inputs(shape, F)
        ref = c["ref"]
        em, off = S.padded_loop_reference(c["lengths"], c["gt"], c["mu"], c["lv"], c["x"], c["y"])
        assert ref["lengths"].tolist() == list(c["lengths"])
        assert np.abs(ref["em"] - em).max() <= 1e-12 * ref["A"].max()
        assert np.abs(ref["off"] - off).max() <= 1e-12 * max(ref["off"].max(), 1.0)
        assert (ref["A"] >= np.abs(ref["em"])).all() and (ref["off"] >= 0).all()
        assert ref["em"].shape == ref["off"].shape == (len(c["lengths"]),)
    # log-variances of both signs: some segment's NLL is well under its unit
    c = S.abi_inputs("b33t9", 129)["ref"]
    assert (np.abs(c["em"]) < 0.5 * c["A"]).any()


def test_abi_shapes_have_what_they_claim():
    sh = S.ABI_SHAPES
    assert sh["b1t1"] == [1]
    assert sh["ties"].count(7) == 2 and sh["ties"].count(1) == 2
    assert len(sh["b33t9"]) == 33 and max(sh["b33t9"]) == 9 and 9 % 4
    assert len(sh["b97steep"]) == 97 and S.batch_sizes_of(sh["b97steep"]).tolist()[:2] == [97, 1]
    for l in sh.values():
        assert list(l) == sorted(l, reverse=True)
        bs = S.batch_sizes_of(l)
        seg = S.segment_of_rows(bs)
        assert len(seg) == sum(l) and np.bincount(seg).tolist() == list(l)
        assert S.lengths_of(bs).tolist() == list(l)


@pytest.mark.parametrize("name", SMALL_LSTM)
def test_reference_sums_to_oracle_scalars(name):
    """The segmented float64 losses of a fixture's batch add up to the oracle's
    own em / off_loss / digamma_kl (float64, eps = 0, eval mode)."""
    r = S.small_reference(name)
    assert not r["meta"].get("plain")
    sc = r["scores"]
    B = int(r["batch"]["batch_sizes"][0])
    assert sc["em"].shape == sc["off"].shape == sc["rows"].shape == (B,)
    assert abs(sc["em"].sum() - sc["em_total"]) <= 1e-10 * abs(sc["em_total"])
    assert abs(sc["off"].sum() - sc["off_total"]) <= 1e-10 * abs(sc["off_total"])
    kl = sc["prior"] * B / S.N_DATA + sc["rows"].sum()
    assert abs(kl - sc["kl_total"]) <= 1e-9 * max(abs(sc["kl_total"]), 1.0)
    assert sc["lengths"].sum() == r["batch"]["data"].shape[0]


def test_kl_reference_splits_digamma_kl():
    from oracle import abcd_oracle as O
    for name in ("k16", "k128"):
        c = S.kl_inputs(name, 5)
        P = {"feature_sampler/posterior_shape_logits": c["psl"].double(),
             "feature_sampler/prior_concentration": torch.tensor(c["a0"], dtype=torch.float64)}
        kl = float(O.digamma_kl(P, c["logits"].double(), S.N_DATA))
        assert abs(kl - c["ref"]["kl"]) <= 1e-10 * abs(kl)
        assert (c["ref"]["row_unit"] >= np.abs(c["ref"]["rows"])).all()
    c = S.kl_inputs("plain10pad", 5)
    mu, lv = c["logits"][:, :10], c["logits"][:, 16:26]
    assert abs(float(O.gaussian_kl(mu.double(), lv.double())) - c["ref"]["kl"]) <= 1e-10 * abs(c["ref"]["kl"])
    assert float(c["logits"][:, 10:16].abs().max()) == 0.0 == float(c["logits"][:, 26:].abs().max())


def test_new_entry_points_are_declared_bound_and_exported():
    from modules import _native as N
    from test_host import header_symbols
    for s in ("abcd_segment_losses_workspace_bytes", "abcd_segment_losses", "abcd_sampler_kl_rows"):
        assert s in header_symbols() and s in N.EXPORTED and hasattr(N.lib(), s), s
    ws = N.lib().abcd_segment_losses_workspace_bytes
    assert ws(200, 512) >= 201 * 4
    assert ws(0, 4) == 0 and ws(4, 0) == 0 and ws(1 << 20, 4) == 0
    assert (N.SEG_LOSSES, N.KL_ROWS) == (11, 12)
    # host-side argument checks need no GPU: nothing is launched on ABCD_EINVAL
    bs = torch.tensor([2, 3], dtype=torch.int64)  # not non-increasing
    pk = N.Packed(None, bs.data_ptr(), 2, 5, 2, 4)
    assert N.lib().abcd_segment_losses(pk, None, 4, None, 4, None, None, None, None, None, None, 0, None) == \
        N.ABCD_EINVAL


def test_ops_and_methods_exist():
    from modules import model as M, ops
    for name in ("segment_losses", "sampler_kl_rows"):
        assert name in ops.OPS and hasattr(torch.ops.abcd, name)
    assert callable(M.RNN_Variational_Decoder.score) and callable(M.ABCDSampler.kl_rows)
    assert callable(M.Sampler.kl_rows)
    # the fake implementations give the shapes without a device
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        rows, prior = torch.ops.abcd.sampler_kl_rows(torch.empty(4, 16), torch.empty(16), [16, 16, 16, 16, 0, 0, 0],
                                                     1.0, 100.0)
        assert rows.shape == (4,) and prior.shape == ()
    schema = str(torch.ops.abcd.segment_losses.default._schema)
    assert schema.startswith("abcd::segment_losses(Tensor? gt, Tensor batch_sizes, Tensor? mu, Tensor? log_var, "
                             "Tensor? offset_logits, Tensor? gt_offset, SymInt F) -> Tensor[]"), schema
    dec = M.RNN_Variational_Decoder(33, 32, 32, 32)
    with pytest.raises(RuntimeError):  # no CPU fallback
        dec.score(torch.zeros(2, 32), torch.tensor([2, 1]), ground_truth_out=torch.zeros(3, 33))
    with pytest.raises(ValueError):
        dec.score(torch.zeros(2, 32), torch.tensor([2, 1]))
    with pytest.raises(RuntimeError):
        M.ABCDSampler(32, 32, 16, 32).kl_rows(torch.zeros(2, 16), 100)


def test_score_cli_arguments():
    import score
    a = score.get_parameters(["ckpt.pt", "root", "ann.csv", "1.0"])
    assert (a.model_path, a.input_root, a.annotation_file, a.data_normalizer) == ("ckpt.pt", "root", "ann.csv", 1.0)
    assert a.mean and not a.sample and a.samples == 1 and a.seed is None and a.device == "cuda"
    assert a.batch_size == 1 and a.save_path is None and a.epsilon == 2 ** -15
    a = score.get_parameters(["c", "r", "a", "2.5", "--sample", "--samples", "3", "--seed", "7", "-b", "4", "-d",
                              "cuda:1", "-S", "out.csv"])
    assert a.sample and not a.mean and (a.samples, a.seed, a.batch_size, a.device, a.save_path) == \
        (3, 7, 4, "cuda:1", "out.csv")
    a = score.get_parameters(["c", "r", "a", "1", "--samples", "2"])  # S > 1 implies sampling
    assert a.sample and not a.mean
    a = score.get_parameters(["c", "r", "a", "1", "--mean"])
    assert a.mean and not a.sample
    for bad in (["--mean", "--sample"], ["--mean", "--samples", "2"], ["--samples", "0"]):
        with pytest.raises(SystemExit):
            score.get_parameters(["c", "r", "a", "1"] + bad)
    # the same data arguments as encode.py
    import encode
    e = vars(encode.get_parameters(["c", "r", "a", "1"]))
    s = vars(score.get_parameters(["c", "r", "a", "1"]))
    assert set(e) <= set(s) and all(s[k] == e[k] for k in e)


def _toy_dataset():
    from modules import data_utils
    from modules.data_utils import Compose
    parser = data_utils.Data_Parser(TOY, ANN)
    fs = parser.get_sample_freq()
    tfm = Compose([data_utils.ToTensor(), data_utils.STFT(int(np.floor(0.008 * fs)), int(np.floor(0.004 * fs))),
                   data_utils.Transform(lambda x: (x + 2 ** -15).log() / 1.0)])
    return parser.get_data(transform=tfm)


def test_score_table_writer_with_stub_scorer(tmp_path):
    """score_table with a scorer that returns known per-row values: one row per
    segment, rows mapped back to data_ix through the loader's in-batch sort,
    total = the sum of the four terms, the annotation columns appended, an
    earlier table kept as .prev, and nothing left behind by a failing run."""
    import score
    ds = _toy_dataset()
    n = len(ds)

    def stub(packed, is_offset, speaker):
        seqs = torch.nn.utils.rnn.unpack_sequence(packed)
        lens = torch.tensor([s.shape[0] for s in seqs])
        assert lens.tolist() == sorted(lens.tolist(), reverse=True)  # packed row order
        first = torch.stack([s[0, 0] for s in seqs]).double()
        return {"length": lens, "category_ix": lens % 16, "emission_nll": first, "end_prediction_loss": first * 2,
                "kl_row": first * 4, "kl_prior_share": torch.full_like(first, 0.125)}

    out = os.path.join(str(tmp_path), "sub", "scores.csv")
    os.makedirs(os.path.dirname(out))
    done = []
    assert score.score_table(stub, ds, out, batch_size=3, finish=lambda: done.append(1)) == n
    assert done == [1]
    df = pd.read_csv(out)
    ann = pd.read_csv(ANN)
    assert list(df.columns) == list(score.COLUMNS) + ["onset", "offset", "input_path", "data_type", "speaker", "label"]
    assert sorted(df["data_ix"].tolist()) == list(range(n)) and len(df) == n
    for _, row in df.iterrows():
        ix = int(row["data_ix"])
        seq, _ = ds[ix]
        assert row["length"] == seq.shape[0] and row["category_ix"] == seq.shape[0] % 16
        assert row["emission_nll"] == pytest.approx(float(seq[0, 0]), rel=1e-12)
        assert row["total"] == pytest.approx(7 * float(seq[0, 0]) + 0.125, rel=1e-9)
        assert row["label"] == ann["label"][ix] and row["onset"] == pytest.approx(ann["onset"][ix])
    # a rerun keeps the earlier table; a failing scorer leaves nothing partial and the table untouched
    score.score_table(stub, ds, out, batch_size=8)
    assert sorted(os.listdir(os.path.dirname(out))) == ["scores.csv", "scores.csv.prev"]

    def failing(packed, is_offset, speaker):
        raise RuntimeError("device lost")
    with pytest.raises(RuntimeError):
        score.score_table(failing, ds, out, batch_size=3)
    assert sorted(os.listdir(os.path.dirname(out))) == ["scores.csv", "scores.csv.prev"]
    assert len(pd.read_csv(out)) == n
