"""What the command-line tools share (``cli.py``), checked on the CPU: outputs
that take their place only when everything is written, the one argument
interface, the featurisation the arguments describe and the annotation join."""
import argparse
import os
import types

import numpy as np
import pandas as pd
import pytest
import torch

import cli

TOY = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "toy_data")
ANN = os.path.join(TOY, "annotation_20170806-080002_89.2-94.22.csv")


def _write(path, text):
    with open(path, "w") as f:
        f.write(text)


def _read(path):
    with open(path) as f:
        return f.read()


def test_replacing_outputs_single_file(tmp_path):
    out = str(tmp_path / "table.csv")
    _write(out, "first")
    _write(out + ".prev", "zeroth")
    with cli.replacing_outputs() as tmp:
        t = tmp(out)
        assert t != out and tmp(out) == t  # one temporary per path: appends go to the same file
        _write(t, "second")
        assert _read(out) == "first"
    assert sorted(os.listdir(tmp_path)) == ["table.csv", "table.csv.prev", "table.csv.prev.prev"]
    assert (_read(out), _read(out + ".prev"), _read(out + ".prev.prev")) == ("second", "first", "zeroth")

    class Failure(Exception):
        pass

    with pytest.raises(Failure):
        with cli.replacing_outputs() as tmp:
            _write(tmp(out), "third")
            raise Failure
    assert sorted(os.listdir(tmp_path)) == ["table.csv", "table.csv.prev", "table.csv.prev.prev"]
    assert (_read(out), _read(out + ".prev"), _read(out + ".prev.prev")) == ("second", "first", "zeroth")
    with pytest.raises(KeyboardInterrupt):  # not only Exception
        with cli.replacing_outputs() as tmp:
            _write(tmp(out), "third")
            raise KeyboardInterrupt
    assert sorted(os.listdir(tmp_path)) == ["table.csv", "table.csv.prev", "table.csv.prev.prev"]
    assert _read(out) == "second"


def test_replacing_outputs_several_files(tmp_path):
    a, b, c, z = (str(tmp_path / n) for n in ("a.csv", "b.wav", "c.csv", "z.npz"))
    _write(a, "old a")
    _write(c, "old c")
    with cli.replacing_outputs() as tmp:
        _write(tmp(a), "new a")
        assert _read(a) == "old a" and not os.path.exists(a + ".prev")
        _write(tmp(b), "new b")
        tmp(c)  # registered, never written: an empty dataset's table
        tz = tmp(z, ext=".npz")
        assert tz.endswith(".npz") and tz != z
        np.savez(tz, x=np.arange(3))
        assert os.listdir(tmp_path).count(os.path.basename(tz)) == 1  # savez wrote that name, not name + .npz
        # nothing has moved yet
        assert _read(a) == "old a" and not os.path.exists(b) and not os.path.exists(z)
        assert not any(n.endswith(".prev") for n in os.listdir(tmp_path))
    assert sorted(os.listdir(tmp_path)) == ["a.csv", "a.csv.prev", "b.wav", "c.csv", "z.npz"]
    assert (_read(a), _read(a + ".prev"), _read(b), _read(c)) == ("new a", "old a", "new b", "old c")
    with np.load(z) as got:
        assert got["x"].tolist() == [0, 1, 2]

    with pytest.raises(ZeroDivisionError):
        with cli.replacing_outputs() as tmp:
            _write(tmp(a), "newer a")
            np.savez(tmp(z, ext=".npz"), x=np.zeros(1))
            tmp(c)
            1 / 0
    assert sorted(os.listdir(tmp_path)) == ["a.csv", "a.csv.prev", "b.wav", "c.csv", "z.npz"]
    assert (_read(a), _read(a + ".prev"), _read(c)) == ("new a", "old a", "old c")
    with np.load(z) as got:
        assert got["x"].tolist() == [0, 1, 2]


def test_one_data_interface():
    import classify
    import encode
    import plain_encode
    import score
    import segment
    import sequence
    base = ["c", "r", "t", "1"]
    shared = {"model_path": "c", "input_root": "r", "data_normalizer": 1.0, "annotation_sep": ",", "device": "cuda",
              "save_path": None, "fft_frame_length": 0.008, "fft_step_size": 0.004, "fft_window_type": "hann_window",
              "fft_no_centering": False, "channel": 0, "epsilon": 2 ** -15}
    for mod in (encode, plain_encode, score, classify, sequence):
        a = vars(mod.get_parameters(base))
        want = dict(shared, annotation_file="t", batch_size=1)
        assert {k: a[k] for k in want} == want, mod.__name__
        assert all(type(a[k]) is type(v) for k, v in want.items()), mod.__name__
    assert set(vars(encode.get_parameters(base))) == set(shared) | {"annotation_file", "batch_size"}
    s = vars(segment.get_parameters(base + ["--max_length", "5"]))
    assert {k: s[k] for k in shared} == shared and s["recording_table"] == "t"
    assert "annotation_file" not in s and "batch_size" not in s
    # the prior arguments: one definition, one check
    for mod, argv in ((classify, base), (sequence, base), (segment, base + ["--max_length", "5"])):
        a = mod.get_parameters(argv)
        assert (a.prior, a.entire_data_size) == ("dirichlet", None)
        for bad in (["--prior", "flat"], ["--entire_data_size", "0"], ["--entire_data_size", "nan"]):
            with pytest.raises(SystemExit):
                mod.get_parameters(argv + bad)
    assert classify.PRIORS is cli.PRIORS and encode.rename_existing_file is cli.rename_existing_file


def _stft_arguments(argv=()):
    p = argparse.ArgumentParser()
    p.add_argument("data_normalizer", type=float)
    cli.add_stft_arguments(p)
    return p.parse_args(["3.5", *argv])


def test_frame_hop_and_log_spectrum():
    from modules import data_utils
    a = _stft_arguments()
    assert cli.frame_hop(a, 16000) == (128, 64)
    assert cli.frame_hop(a, 22050) == (176, 88)  # 176.4 and 88.2 samples: floored
    assert all(type(v) is int for v in cli.frame_hop(a, 22050))
    x = torch.randn(1000, generator=torch.Generator().manual_seed(0)) * 1000.0
    for argv, centering in (((), True), (("--fft_no_centering",), False)):
        a = _stft_arguments(argv + ("-E", "0.25"))
        got = cli.log_spectrum(a, 176, 88)(x)
        want = (data_utils.STFT(176, 88, centering=centering)(x) + 0.25).log() / 3.5
        assert got.shape == (1 + (1000 if centering else 1000 - 176) // 88, 89)
        assert torch.equal(got, want)


def test_open_dataset_is_the_loaders_log_spectrum():
    from modules import data_utils
    p = argparse.ArgumentParser()
    cli.add_data_arguments(p, table_help="", save_help="")
    a = p.parse_args(["ckpt.pt", TOY, ANN, "2.0"])
    ds = cli.open_dataset(a)
    parser = data_utils.Data_Parser(TOY, ANN)
    fs = parser.get_sample_freq()
    frame, hop = int(np.floor(0.008 * fs)), int(np.floor(0.004 * fs))
    tfm = data_utils.Compose([data_utils.ToTensor(), data_utils.STFT(frame, hop),
                              data_utils.Transform(lambda x: (x + 2 ** -15).log() / 2.0)])
    ref = parser.get_data(transform=tfm)
    assert len(ds) == len(ref) == 8
    for ix in (0, 7):
        assert torch.equal(ds[ix][0], ref[ix][0]) and ds[ix][1] == ref[ix][1]


def test_join_annotation(tmp_path):
    from modules import data_utils
    ds = data_utils.Data_Parser(TOY, ANN).get_data()
    ann = cli.annotation_columns(ds)
    assert list(ann.columns) == ["onset", "offset", "input_path", "data_type", "speaker", "label"]
    assert {"onset_ix", "offset_ix", "length"} <= set(ds.df_annotation.columns)  # (the dataset's own are left)
    ix = np.array([5, 0, 7, 2, 2])
    table = pd.DataFrame({"data_ix": ix, "value": np.arange(5.0)})
    got = cli.join_annotation(table, ann)
    assert list(got.columns) == ["data_ix", "value"] + list(ann.columns)
    assert got["data_ix"].tolist() == ix.tolist() and got["value"].tolist() == [0.0, 1.0, 2.0, 3.0, 4.0]
    src = pd.read_csv(ANN)
    assert got["label"].tolist() == src["label"].to_numpy()[ix].tolist() == ["B", "A", "A", "B", "B"]
    assert got["speaker"].tolist() == src["speaker"].to_numpy()[ix].tolist()
    assert got["onset"].tolist() == src["onset"].to_numpy()[ix].tolist()
    assert list(got.index) == list(range(5))
    # no label column: nothing to join
    bare = str(tmp_path / "bare.csv")
    src.drop(columns=["label"]).to_csv(bare, index=False)
    assert cli.annotation_columns(data_utils.Data_Parser(TOY, bare).get_data()) is None
    assert cli.join_annotation(table, None) is table
    # an annotation that never had the dataset's index columns
    only = cli.annotation_columns(types.SimpleNamespace(df_annotation=src[["label", "onset"]]))
    assert list(only.columns) == ["label", "onset"]
