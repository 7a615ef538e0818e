#!/usr/bin/env python3
"""Assemble profiles/parity_errors.json from one GPU suite run.

    ABCD_PARITY_DUMP=<dir> python -m pytest -m gpu tests
    python scripts/parity_table.py <dir>

tests/test_gpu_edges.py, test_gpu_ladder.py, test_gpu_decoder_noise.py, test_gpu_fullshape.py,
test_gpu_prod.py, test_gpu_sampler_widths.py and test_gpu_philox.py write the errors they
observed (the HIP path against the float64 / fp32 oracle or the reference's
fixtures) into <dir> when ABCD_PARITY_DUMP is set; this puts them into one
table next to the tolerances derived from them (what other test files
dump there belongs to other tables and is left alone).  A section <dir> holds no
figures for (a run of some of the files) keeps what the table has.
"""
import glob
import json
import os
import re
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))


def sig(x, n=3):
    return float(f"{x:.{n - 1}e}")


def main(src):
    import edge_cases as E
    import test_gpu_decoder_noise as TN
    import test_gpu_edges as TE
    import test_gpu_fullshape as TF
    import test_gpu_ladder as TL
    import test_gpu_prod as TP
    import test_gpu_sampler_widths as TS
    edges, full, prod, samp, philox, ladder = {}, {}, {}, {}, {}, {}
    worst_ratio, samp_ratio, ladder_ratio = {}, {}, {}
    noise, noise_ratio = {}, {}
    for path in sorted(glob.glob(os.path.join(src, "*.json"))):
        name = os.path.basename(path)[:-5]
        with open(path) as f:
            d = json.load(f)
        if name.startswith("samp-"):
            rows = {}
            for r in d:
                k = r["tensor"]
                rows[k] = [sig(r["e32_rel"]), sig(r["e_hip_rel"]), sig(r["e32_blk"]), sig(r["e_hip_blk"]), r["R"]]
                for a, b in ((r["e_hip_rel"], r["e32_rel"]), (r["e_hip_blk"], r["e32_blk"])):
                    if r["R"] is not None and a > TS.R_DEFAULT * b + 1e-7:  # past the default bound
                        key = f"{name[len('samp-'):]}: {k}"
                        samp_ratio[key] = max(samp_ratio.get(key, 0.0), sig(a / max(b, 1e-30)))
            samp[name[len("samp-"):]] = rows
        elif name.startswith("ladder-"):
            rows = {}
            for r in d:
                k = r["tensor"]
                rows[k] = [sig(r["e32_rel"]), sig(r["e_hip_rel"]), sig(r["e32_blk"]), sig(r["e_hip_blk"]), r["R"]]
                for a, b in ((r["e_hip_rel"], r["e32_rel"]), (r["e_hip_blk"], r["e32_blk"])):
                    raised = TL.R_ENCODER if name.startswith("ladder-enc-") else TL.R_TENSOR
                    # past the default bound, or a raised tensor's ratio past 4 inside the bound's 1e-7
                    if a > TL.bound(TL.R_DEFAULT, b) or (k in raised and a > TL.R_DEFAULT * b):
                        key = ("encoder: " if name.startswith("ladder-enc-") else "") + k
                        if sig(a / max(b, 1e-30)) > ladder_ratio.get(key, (0.0, ""))[0]:
                            ladder_ratio[key] = (sig(a / max(b, 1e-30)), name[len("ladder-"):])
            ladder[name[len("ladder-"):]] = rows
        elif name.startswith("noise-"):
            rows = {}
            for r in d:
                k = r["tensor"]
                rows[k] = [sig(r["e32_rel"]), sig(r["e_hip_rel"]), sig(r["e32_blk"]), sig(r["e_hip_blk"]), r["R"]]
                for a, b in ((r["e_hip_rel"], r["e32_rel"]), (r["e_hip_blk"], r["e32_blk"])):
                    if a > TL.bound(TL.R_DEFAULT, b):  # past the default bound
                        key = ("encoder: " if name.startswith("noise-encdrop-") else "") + k
                        if sig(a / max(b, 1e-30)) > noise_ratio.get(key, (0.0, ""))[0]:
                            noise_ratio[key] = (sig(a / max(b, 1e-30)), name[len("noise-"):])
            noise[name[len("noise-"):]] = rows
        elif name.startswith("philox-"):
            philox[name[len("philox-"):]] = {k: (sig(v) if isinstance(v, float) else v) for k, v in d[0].items()}
        elif name.startswith("fullshape-"):
            full[name[len("fullshape-"):]] = dict(
                clip=sig(d["clip"]), worst={m: sig(x) for m, x in d["worst"].items()},
                tensors={k: {m: sig(x) for m, x in v.items()} for k, v in d["tensors"].items()})
        elif name.startswith("prod-"):
            prod[name[len("prod-"):]] = dict(
                worst=sig(d["worst"]), **({"clip": sig(d["clip"])} if "clip" in d else {}),
                tensors={k: {m: sig(x) for m, x in v.items()} for k, v in d.get("tensors", {}).items()})
        elif name.split("-")[0] in E.CASES:  # test_gpu_edges.py: <case>-<widths> / <case>-frames
            rows = {}
            for r in d:
                rows[r["tensor"]] = [sig(r["e32_rel"]), sig(r["e_hip_rel"]), sig(r["e32_blk"]), sig(r["e_hip_blk"]), r["R"]]
                k = r["tensor"]
                for a, b in ((r["e_hip_rel"], r["e32_rel"]), (r["e_hip_blk"], r["e32_blk"])):
                    if a > TE.bound(k, b, R=TE.R_DEFAULT):  # past the default bound
                        worst_ratio[k] = max(worst_ratio.get(k, 0.0), sig(a / max(b, 1e-30)))
            edges[name] = rows
    table = {
        "what": "errors of the HIP path observed in one `pytest -m gpu tests` run on MI355X (scripts/parity_table.py)",
        "edge_cases": {
            "columns": ["e32_rel", "e_hip_rel", "e32_blk", "e_hip_blk", "R"],
            "metrics": "rel = max|a - ref| / max|ref|; blk = edge_cases.block_err (worst 16 x 16 block, floor 1e-2); "
                       "ref = the float64 oracle; e32 = the fp32 oracle, e_hip = the GPU. g/ gradients, d/ post-SGD "
                       "deltas (e32 = the gradient's + the norm's; the stored parameter's half-ulp taken off e_hip), "
                       "norm = the clip norm (relative)",
            "bound": "e_hip <= R * e32 + 1e-7, and e_hip <= %g whatever R" % TE.HARD,
            "R_default": TE.R_DEFAULT, "R_tensor": TE.R_TENSOR,
            "worst_ratio_past_R_default": worst_ratio,
            "R_note": "R is raised only for a tensor past the default bound, to at most 2 x its own worst ratio. "
                      + TE.R_NOTE,
            "worst_e_hip": {m: max(r[i] for rows in edges.values() for r in rows.values())
                            for m, i in (("rel", 1), ("blk", 3))} if edges else {},
            "cases": edges,
        },
        "ladder": {
            "file": "tests/test_gpu_ladder.py (widths, routes and references: tests/ladder_cases.py)",
            "reference": "enc-*: torch.nn.LSTM / GRU in float64, e32 the same module in fp32; dec-* / frames-*: the "
                         "float64 oracle step, e32 the fp32 oracle",
            "columns": ["e32_rel", "e_hip_rel", "e32_blk", "e_hip_blk", "R"],
            "bound": "e_hip <= R * e32 + 1e-7, and e_hip <= %g whatever R" % TL.HARD,
            "R_default": TL.R_DEFAULT, "R_tensor": TL.R_TENSOR, "R_encoder": TL.R_ENCODER,
            "worst_ratio_past_R_default": {k: list(v) for k, v in sorted(ladder_ratio.items())},
            "R_note": "R is raised only for a tensor whose e_hip / e32 went past 4, to at most 2 x its own worst "
                      "ratio. " + TL.R_NOTE,
            "worst_e_hip": {m: max(r[i] for rows in ladder.values() for r in rows.values())
                            for m, i in (("rel", 1), ("blk", 3))} if ladder else {},
            "cases": ladder,
        },
        "decoder_noise": {
            "file": "tests/test_gpu_decoder_noise.py (cases, masks, streams and references: tests/noise_cases.py)",
            "reference": "mask-* / maskframes-*: the float64 oracle step fed the replayed input-dropout mask; philox-*: "
                         "the float64 oracle step fed abcd_fill_normal / abcd_fill_dropout's values of the step's "
                         "(seed, offset); encdrop-*: oracle.encoder_forward(hmask=...) with autograd in float64; e32 "
                         "the same in fp32",
            "columns": ["e32_rel", "e_hip_rel", "e32_blk", "e_hip_blk", "R"],
            "bound": "e_hip <= R * e32 + 1e-7, and e_hip <= %g whatever R" % TL.HARD,
            "R_default": TL.R_DEFAULT,
            "R_imported": "test_gpu_edges.R_TENSOR (rung1), test_gpu_ladder.R_TENSOR (the other rows) and "
                          "test_gpu_ladder.R_ENCODER (encdrop), unchanged",
            "R_step": TN.R_STEP, "R_enc": TN.R_ENC,
            "worst_ratio_past_R_default": {k: list(v) for k, v in sorted(noise_ratio.items())},
            "R_note": "R is raised only for a tensor past its bound here, to at most 2 x its own worst ratio. " + TN.R_NOTE,
            "worst_e_hip": {m: max(r[i] for rows in noise.values() for r in rows.values())
                            for m, i in (("rel", 1), ("blk", 3))} if noise else {},
            "cases": noise,
        },
        "full_shape": {
            "file": "tests/test_gpu_fullshape.py", "reference": "the fp32 oracle (oracle.train_step)",
            "metrics": "rel / blk / norm: a gradient against the oracle's; sgd: the post-SGD delta less the stored "
                       "parameter's 2 ulp; clip: the global norm",
            "GRAD_TOL": TF.GRAD_TOL, "BLOCK_TOL": TF.BLOCK_TOL, "GRAD_TOL_before": 1e-3,
            "derivation": "3 x the worst observed in the file, rounded up to one significant digit",
            "worst": {m: max(c["worst"][m] for c in full.values()) for m in ("rel", "blk", "norm", "sgd")} if full else {},
            "cases": full,
        },
        "prod_fixtures": {
            "file": "tests/test_gpu_prod.py", "reference": "tests/golden/prod_*.npz (the reference's own step)",
            "metrics": "every figure GRAD_TOL multiplies: gradient norm, whole gradient (rel), row / column sums, "
                       "post-SGD delta norm and sum",
            "GRAD_TOL": TP.GRAD_TOL, "GRAD_TOL_before": 1e-3,
            "derivation": "3 x the worst observed in the file, rounded up to one significant digit",
            "worst": max(c["worst"] for c in prod.values()) if prod else None,
            "cases": prod,
        },
        "sampler_widths": {
            "file": "tests/test_gpu_sampler_widths.py, tests/test_gpu_philox.py",
            "reference": "the float64 oracle on the un-padded model (tests/sampler_cases.py)",
            "columns": ["e32_rel", "e_hip_rel", "e32_blk", "e_hip_blk", "R"],
            "bound": "e_hip <= R * e32 + 1e-7, and e_hip <= %g whatever R; R null: recorded only, under the "
                     "hard bound alone (in-kernel Gumbel noise: the device's fast log)" % TS.HARD,
            "R_default": TS.R_DEFAULT, "R_case_tensor": {f"{c}: {k}": r for (c, k), r in TS.R_TENSOR.items()},
            "worst_ratio_past_R_default": samp_ratio,
            "R_note": TS.R_NOTE,
            "worst_e_hip": {m: max(r[i] for rows in samp.values() for r in rows.values())
                            for m, i in (("rel", 1), ("blk", 3))} if samp else {},
            "worst_e_hip_per_case": {c: {m: max(r[i] for r in rows.values()) for m, i in (("rel", 1), ("blk", 3))}
                                     for c, rows in samp.items() if rows},
            "fill_normal": philox,
            "cases": samp,
        },
    }
    out = os.path.join(REPO, "profiles", "parity_errors.json")
    # a section <dir> has no figures for keeps what the file holds
    if os.path.isfile(out):
        with open(out) as f:
            old = json.load(f)
        for sec, got in (("edge_cases", edges), ("ladder", ladder), ("decoder_noise", noise), ("full_shape", full), ("prod_fixtures", prod),
                         ("sampler_widths", samp or philox)):
            if not got and sec in old:
                table[sec] = old[sec]
    text = json.dumps(table, indent=1)
    # one line per tensor: collapse the arrays of numbers
    text = re.sub(r"\[\s+([^\[\]{}]*?)\s+\]", lambda m: "[" + re.sub(r"\s+", " ", m.group(1)) + "]", text)
    with open(out, "w") as f:
        f.write(text + "\n")
    print(out, os.path.getsize(out), "bytes;", len(edges), "edge cases,", len(ladder), "ladder cases,", len(full),
          "full-shape,", len(prod), "prod")


if __name__ == "__main__":
    main(sys.argv[1])
