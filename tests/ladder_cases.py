"""The recurrent dispatch ladder off H = Hm = 256, F = 129: widths, batches,
the kernel each one is routed to, and the references it is judged against.

``persist_encoder_fwd / _bwd`` and ``persist_decoder_fwd / _bwd``
(csrc/abcd_persist.hip) pick a kernel template from H, Hm, the padded frame
width Fp, the cell type and whether the decoder feeds its sample back; what
they decline falls to the per-step kernels (csrc/abcd_rnn.hip).  The tables
here name, for each width, the template the ladder's arithmetic selects and the
grid it launches; tests/test_ladder_cases_cpu.py restates that arithmetic, and
tests/test_gpu_ladder.py asserts on the GPU that exactly that kernel ran and
compares it with float64.

Every H, Hm and D is a multiple of 16 (modules/padding.py is not involved).
Batches are ``edge_cases.CASES`` (T <= 12); these forms work in 64-row tiles
(``PERSIST_ROWS``), so ``b65`` / ``b97steep`` cross their tile boundary and
``b160`` is three tiles with a ragged one.  The batch helpers, the oracle
step and the error metrics are those of tests/edge_cases.py.
"""
import functools
from collections import OrderedDict

import torch

import edge_cases as E

SEED = 1
ROWS = 64           # PERSIST_ROWS: rows per workgroup of the forms tested here
LDS_LIMIT = 160 * 1024


def cdiv(a, b):
    return -(-a // b)


def gates(rnn):
    return 4 if rnn == "LSTM" else 3


# ----------------------------------------------------------------------------
# encoder widths (F = 33, Fp = 48): H -> (forward, {rnn: backward}); "%d" = G
# ----------------------------------------------------------------------------
ENC_F = 33
ENC_ROUTES = OrderedDict([
    (16, ("enc_fwd_persist<%d,1,0>", {"LSTM": "enc_bwd_persist<4,4>", "GRU": "enc_bwd_persist<3,1>"})),
    (48, ("enc_fwd_persist<%d,1,0>", {"LSTM": "enc_bwd_persist<4,4>", "GRU": "enc_bwd_persist<3,1>"})),
    (64, ("enc_fwd_persist<%d,16,2>", {"LSTM": "enc_bwd_sk<4,4>", "GRU": "enc_bwd_sk<3,4>"})),
    (128, ("enc_fwd_persist<%d,16,4>", {"LSTM": "enc_bwd_sk<4,8>", "GRU": "enc_bwd_sk<3,8>"})),
    (192, ("enc_fwd_persist<%d,4,0>", {"LSTM": "enc_bwd_persist<4,16>", "GRU": "enc_bwd_persist<3,4>"})),
    # the only width on the non-x6 depth-16 forward ring: 128 KiB of weights in LDS, 32 members per group
    (512, ("enc_fwd_persist<%d,16,0>", {"LSTM": "enc_bwd_persist<4,16>", "GRU": "enc_bwd_persist<3,16>"})),
    # as the encoder side of a decoder row only: H = 32 (2 chunks: the rings of H = 16 / 48), and
    # H = 256, the rung tests/test_gpu_edges.py covers
    (32, ("enc_fwd_persist<%d,1,0>", {"LSTM": "enc_bwd_persist<4,4>", "GRU": "enc_bwd_persist<3,1>"})),
    (256, ("enc_fwd_persist<%d,16,8>", {"LSTM": "enc_bwd_w8<4>", "GRU": "enc_bwd_w8<3>"})),
])
ENC_WIDTHS = [H for H in ENC_ROUTES if H not in (32, 256)]
BASE_BATCHES = ("b65", "b97steep")
EXTRA_BATCHES = ("b1t1", "b160")
# one width per distinct forward template for the extra batches (H = 16 shares <G,1,0> with H = 48)
ENC_EXTRA_WIDTHS = (48, 64, 128, 192, 512)
ENC_CASES = [(H, rnn, b) for H in ENC_WIDTHS for rnn in ("LSTM", "GRU") for b in BASE_BATCHES] + \
    [(H, rnn, b) for H in ENC_EXTRA_WIDTHS for rnn in ("LSTM", "GRU") for b in EXTRA_BATCHES]
# (H, layers, bidirectional): LSTM, b65
ENC_VARIANTS = [(48, 2, True), (48, 1, False), (128, 2, True), (128, 1, False)]


def enc_grid(H, B, rnn, nd=2):
    """Workgroups of an encoder launch: directions x row groups x members.
    Every form here has H / 16 members on 64-row groups but enc_bwd_w8 (H = 256:
    8 members on 32-row groups) -- returned as (forward, backward)."""
    fwd = nd * cdiv(B, ROWS) * (H // 16)
    return fwd, (nd * cdiv(B, 32) * 8 if H == 256 else fwd)


def enc_expected(H, rnn, B, nd=2):
    """{role: dispatch string} of one encoder layer."""
    fwd, bwd = ENC_ROUTES[H]
    gf, gb = enc_grid(H, B, rnn, nd)
    return {"enc_fwd": f"{fwd % gates(rnn)} grid {gf}", "enc_bwd": f"{bwd[rnn]} grid {gb}"}


# ----------------------------------------------------------------------------
# decoder rows: a full training step, encoder H = decoder H
# ----------------------------------------------------------------------------
X6F, W16, PER = "dec_fwd_x6<%d,8,8,{rnn}>", "dec_bwd_w16<%d,{rnn}>", "dec_fwd_persist<%d>"
STEP_F, STEP_B = "per-step decoder forward<%d>", "per-step decoder backward<%d>"
# name -> dims, flags, and per cell type (forward, backward); a cell type without an entry has no case
DEC_ROWS = OrderedDict([
    ("f65", dict(F=65, H=256, Hm=256, routes={"LSTM": (X6F % 11, W16 % 5), "GRU": (X6F % 11, W16 % 5)})),
    ("greedy", dict(F=129, H=256, Hm=256, greedy=True,
                    routes={"LSTM": (X6F % 8, W16 % 0), "GRU": (X6F % 8, W16 % 0)})),
    ("hm128", dict(F=129, H=256, Hm=128, routes={"LSTM": (PER % 13, "dec_bwd_persist"),
                                                 "GRU": (STEP_F % 3, STEP_B % 3)})),
    ("hm128g", dict(F=129, H=256, Hm=128, greedy=True, routes={"LSTM": (PER % 8, "dec_bwd_persist")})),
    # 2 x 17 > 32 emit tiles: no x6 / split-K form.  The backward gather form needs
    # cdiv(17 + 16, 32) = 2 gate images of 64 KiB + 17 + 32 KiB = 177 KiB of LDS: over the
    # 160 KiB a workgroup has, so fits_resident declines it and the BPTT runs per step
    ("f257", dict(F=257, H=256, Hm=256, routes={"LSTM": (PER % 0, STEP_B % 4), "GRU": (STEP_F % 3, STEP_B % 3)})),
    # 8 members for 6 mlp and 3 emit tiles: some members idle
    ("h64", dict(F=33, H=64, Hm=48, routes={"LSTM": (PER % 0, "dec_bwd_persist"), "GRU": (STEP_F % 3, STEP_B % 3)})),
    # 4 members for 10 mlp and 9 emit tiles: n1 = n2 = 3, ragged shares
    ("h32", dict(F=129, H=32, Hm=80, routes={"LSTM": (PER % 0, "dec_bwd_persist")})),
    # ABCD_PERSIST=0: all four per-step fallbacks
    ("stepwise", dict(F=33, H=48, Hm=32, persist=False, routes={"LSTM": (STEP_F % 4, STEP_B % 4)})),
])
DEC_D, DEC_K = 32, 16
# the rows that run the extra batches: one per distinct decoder kernel name
DEC_EXTRA = [("f65", "LSTM"), ("f65", "GRU"), ("greedy", "LSTM"), ("greedy", "GRU"), ("hm128", "LSTM"),
             ("hm128", "GRU"), ("hm128g", "LSTM"), ("h32", "LSTM"), ("stepwise", "LSTM")]
DEC_CASES = [(row, rnn, b) for row, d in DEC_ROWS.items() for rnn in d["routes"] for b in BASE_BATCHES] + \
    [(row, rnn, b) for row, rnn in DEC_EXTRA for b in EXTRA_BATCHES]
FRAME_CASES = [("f65", "LSTM", "b65"), ("hm128", "LSTM", "b65"), ("h32", "LSTM", "b65")]

# gradients that are identically zero in exact arithmetic, beyond edge_cases.ZERO_GRADS: a greedy
# decoder's input is x * 0 in training, so the cell's input weights get no gradient
GREEDY_ZERO = {"decoder/rnn_cell.cell.weight_ih"}


def dec_grid(kernel, H, B):
    """Workgroups of a decoder launch (None: a per-step string carries no
    grid).  dec_bwd_w16: 16 members on 32-row groups; the other persistent
    forms: H / 8 members on 64-row groups."""
    if kernel.startswith("per-step"):
        return None
    if kernel.startswith("dec_bwd_w16"):
        return cdiv(B, 32) * 16
    return cdiv(B, ROWS) * (H // 8)


def dec_expected(row, rnn, B):
    """{role: dispatch string} of one training step of a decoder row, all four roles."""
    d = DEC_ROWS[row]
    if d.get("persist", True):
        exp = enc_expected(d["H"], rnn, B)
    else:
        G = gates(rnn)
        exp = {"enc_fwd": "per-step rnn_fwd_step<%d>" % G, "enc_bwd": "per-step launch_bwd_step<%d>" % G}
    for role, kern in zip(("dec_fwd", "dec_bwd"), d["routes"][rnn]):
        kern = kern.format(rnn=rnn)
        g = dec_grid(kern, d["H"], B)
        exp[role] = kern if g is None else f"{kern} grid {g}"
    return exp


def dec_config(row, rnn, B):
    """A row's configuration in bench.CONFIGS' keys (what edge_cases.make_batch / oracle_cfg read)."""
    d = DEC_ROWS[row]
    return dict(F=d["F"], H=d["H"], Hm=d["Hm"], D=DEC_D, K=DEC_K, rnn=rnn, plain=False, spk=0, sdim=None, B=B,
                greedy=d.get("greedy", False), persist=d.get("persist", True))


def meta_of(cfg, layers=1, bidirectional=True):
    """The fixture-style description gpu_helpers.build_from_meta builds modules from."""
    return dict(dims=dict(F=cfg["F"], H=cfg["H"], Hm=cfg["Hm"], D=cfg["D"], K=cfg["K"]), rnn=cfg["rnn"],
                greedy=cfg.get("greedy", False), layers=layers, bidirectional=bidirectional)


def arrays_of(P):
    """Oracle parameters keyed the way a fixture's arrays are (``p/<name>``)."""
    return {"p/" + k: v for k, v in P.items()}


@functools.lru_cache(maxsize=None)
def dec_reference(row, rnn, case):
    """Everything the tests of one decoder (row, rnn, batch) share, computed
    once and never modified: configuration, seed-1111 oracle weights, the
    batch and its noise, the float64 and fp32 oracle steps."""
    from oracle import abcd_oracle as O
    lengths = E.CASES[case]
    cfg = dec_config(row, rnn, len(lengths))
    ocfg = dict(E.oracle_cfg(cfg), greedy=cfg["greedy"])
    P = O.init_params(ocfg, 1111)
    batch, noise = E.make_batch(lengths, cfg, SEED)
    r64 = E.oracle64(ocfg, P, batch, noise, E.N_DATA)
    r32 = E.oracle32(ocfg, P, batch, noise, E.N_DATA)
    return dict(cfg=cfg, ocfg=ocfg, P=P, batch=batch, noise=noise, r64=r64, r32=r32)


def zero_grads(row, case):
    z = set(E.ZERO_GRADS.get(case, set()))
    return z | GREEDY_ZERO if DEC_ROWS[row].get("greedy") else z


# ----------------------------------------------------------------------------
# the encoder alone against torch.nn.LSTM / GRU
# ----------------------------------------------------------------------------
def enc_config(H, rnn, B):
    return dict(F=ENC_F, H=H, Hm=32, D=DEC_D, K=DEC_K, rnn=rnn, plain=False, spk=0, sdim=None, B=B)


def _torch_rnn(P, cfg, layers, bidirectional, dtype):
    cls = torch.nn.LSTM if cfg["rnn"] == "LSTM" else torch.nn.GRU
    ref = cls(cfg["F"], cfg["H"], layers, bidirectional=bidirectional, batch_first=True).to(dtype)
    with torch.no_grad():
        for n, p in ref.named_parameters():
            p.copy_(P["encoder/rnn." + n].to(dtype))
    return ref


def _torch_run(ref, packed, dout, dtype):
    """last_hidden (model.py:60-66: transpose(cat(h_n, c_n, -1), 0, 1).view(B, -1)) and the
    gradients of sum(last_hidden * dout)."""
    for p in ref.parameters():
        p.grad = None
    _, hn = ref(torch.nn.utils.rnn.PackedSequence(packed.data.to(dtype), packed.batch_sizes))
    if isinstance(hn, tuple):
        hn = torch.cat(hn, dim=-1)
    out = hn.transpose(0, 1).contiguous().view(hn.shape[1], -1)
    (out * dout.to(dtype)).sum().backward()
    res = OrderedDict(last_hidden=out.detach())
    res.update(("g/" + n, p.grad.detach().clone()) for n, p in ref.named_parameters())
    return res


@functools.lru_cache(maxsize=None)
def enc_reference(H, rnn, case, layers=1, bidirectional=True):
    """One encoder (H, rnn, batch): oracle-initialised weights, the packed
    batch, a fixed ``dout``, and torch.nn.LSTM / GRU run forward and backward
    in float64 (``r64``) and in fp32 (``r32``, the unit of the GPU's error)."""
    from oracle import abcd_oracle as O
    lengths = E.CASES[case]
    cfg = enc_config(H, rnn, len(lengths))
    ocfg = dict(E.oracle_cfg(cfg), layers=layers, bidirectional=bidirectional)
    P = O.init_params(ocfg, 1111)
    batch, _ = E.make_batch(lengths, cfg, SEED)
    packed = torch.nn.utils.rnn.PackedSequence(batch["data"], batch["batch_sizes"])
    dout = torch.randn(len(lengths), O.encoder_out_size(ocfg), generator=torch.Generator().manual_seed(SEED + 5))
    r64 = _torch_run(_torch_rnn(P, cfg, layers, bidirectional, torch.float64), packed, dout, torch.float64)
    r32 = _torch_run(_torch_rnn(P, cfg, layers, bidirectional, torch.float32), packed, dout, torch.float32)
    e32 = OrderedDict((k, (E.rel_err(r32[k], v), E.block_err(r32[k], v))) for k, v in r64.items())
    return dict(cfg=cfg, ocfg=ocfg, P=P, packed=packed, dout=dout, r64=r64, r32=r32, e32=e32,
                meta=meta_of(cfg, layers, bidirectional))
