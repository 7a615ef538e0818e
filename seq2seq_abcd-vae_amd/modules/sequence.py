# coding: utf-8
"""Context-aware labels: a hidden Markov model whose states are the K
categories and whose emission term is ``classify.py``'s ``-nll[b, k]``
(``ops.chain_scores``).  ``TransitionModel`` holds the chain (``log_trans``,
``log_init``), runs forward-backward and Viterbi through
``torch.ops.abcd.chain_posterior`` and fits the chain by EM; ``split_sequences``
cuts an annotation table into the sequences the chain runs over."""
import numpy as np
import torch

from . import ops


def split_sequences(annotation_frame, by=("input_path",), max_gap=None):
    """Annotation rows -> ``(order, seq_off)``: ``order`` lists the row
    positions sequence by sequence in time order, sequence s owning
    ``order[seq_off[s]:seq_off[s + 1]]``.  Rows are grouped by the ``by``
    columns (groups in sorted key order) and sorted by onset within a group; a
    new sequence starts where the next onset lies more than ``max_gap`` seconds
    after the previous offset (``None``: never).  A pure function of the
    table."""
    df = annotation_frame
    n = len(df)
    if n == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(1, dtype=np.int64)
    pos = np.arange(n, dtype=np.int64)
    onset = np.asarray(df["onset"], dtype=np.float64)
    offset = np.asarray(df["offset"], dtype=np.float64)
    by = [by] if isinstance(by, str) else list(by)
    if by:
        keys = [np.unique(np.asarray(df[c]).astype(str), return_inverse=True)[1] for c in by]
        idx = np.lexsort([pos, onset] + keys[::-1])     # by the keys in column order, then onset, then row position
        key = np.stack([k[idx] for k in keys], 1)
        new = np.r_[True, (key[1:] != key[:-1]).any(1)]
    else:
        idx = np.lexsort([pos, onset])
        new = np.r_[True, np.zeros(n - 1, dtype=bool)]
    if max_gap is not None:
        gap = onset[idx][1:] - offset[idx][:-1]
        new[1:] |= gap > float(max_gap)
    seq_off = np.r_[np.flatnonzero(new), n].astype(np.int64)
    return idx.astype(np.int64), seq_off


class TransitionModel(torch.nn.Module):
    """A first-order chain over K categories: ``log_trans[i, j] = log p(z_t+1 =
    j | z_t = i)`` and ``log_init[k]``, uniform until fitted or loaded.  Every
    method takes ``score`` (N x K on the GPU, each row's maximum at 0:
    ``ops.chain_scores``) and ``seq_off`` (S + 1 row offsets on the host); there
    is no CPU path."""

    def __init__(self, K):
        super().__init__()
        K = int(K)
        if K < 1:
            raise ValueError("TransitionModel: K must be at least 1")
        self.K = K
        self.register_buffer("log_trans", torch.full((K, K), -float(np.log(K))))
        self.register_buffer("log_init", torch.full((K,), -float(np.log(K))))

    @classmethod
    def from_log_weight(cls, lw):
        """The context-free model: every row of the transition matrix and the
        initial distribution equal softmax(lw), so ``posterior`` reproduces
        ``ops.pair_posterior`` with weights lw."""
        lw = torch.as_tensor(lw)
        m = cls(lw.numel()).to(lw.device)
        p = torch.log_softmax(lw.double().reshape(-1), 0).float()
        m.log_init.copy_(p)
        m.log_trans.copy_(p[None, :].expand(m.K, m.K))
        return m

    def set_probabilities(self, trans, init):
        """Load a row-stochastic K x K matrix and an initial distribution."""
        dev = self.log_trans.device
        self.log_trans.copy_(torch.as_tensor(trans, dtype=torch.float64, device=dev).log().float())
        self.log_init.copy_(torch.as_tensor(init, dtype=torch.float64, device=dev).log().float())
        return self

    def _run(self, score, seq_off, want):
        seq_off = torch.as_tensor(seq_off, dtype=torch.int64)
        with torch.no_grad():
            return ops.chain_posterior(score, seq_off, self.log_trans, self.log_init, want)

    def posterior(self, score, seq_off, counts=False):
        """dict(log_evidence S fp64, gamma N x K) and, with ``counts``, the
        expected transition and initial counts (K x K and K, fp64)."""
        want = ops.CHAIN_EVIDENCE | ops.CHAIN_GAMMA | (ops.CHAIN_COUNTS if counts else 0)
        ev, gamma, _, _, tc, ic = self._run(score, seq_off, want)
        out = dict(log_evidence=ev, gamma=gamma)
        if counts:
            out.update(trans_counts=tc, init_counts=ic)
        return out

    def viterbi(self, score, seq_off):
        """(path N int32, path_score S fp64): the most probable state sequence
        of every sequence (the lowest index wins ties; -1 where no path
        exists) and its log joint."""
        _, _, path, ps, _, _ = self._run(score, seq_off, ops.CHAIN_PATH)
        return path, ps

    def objective(self, log_evidence, pseudo_count):
        """sum_s log_evidence_s + c (sum log_trans + sum log_init) over the
        finite entries: the log posterior EM climbs, up to a constant."""
        lt, li = self.log_trans.double(), self.log_init.double()
        pen = lt[torch.isfinite(lt)].sum() + li[torch.isfinite(li)].sum()
        return log_evidence.sum() + float(pseudo_count) * pen

    def fit(self, score, seq_off, n_iter=10, pseudo_count=None):
        """EM: the E-step is one ``chain_posterior`` call, the M-step
        ``(counts + c)`` normalised per row (and the same for the initial
        distribution) in float64 on the device.  Returns the objective after
        every iteration (``n_iter`` floats, non-decreasing; the value before
        the first iteration is kept as ``initial_objective``).  ``last_counts``
        keeps the expected counts of the final E-step that updated the model."""
        c = 1.0 / self.K if pseudo_count is None else float(pseudo_count)
        want = ops.CHAIN_EVIDENCE | ops.CHAIN_COUNTS
        objs = []
        self.last_counts = None
        ev, _, _, _, tc, ic = self._run(score, seq_off, want)
        for _ in range(int(n_iter)):
            objs.append(self.objective(ev, c))
            self.last_counts = (tc, ic)
            t, i = tc + c, ic + c
            self.log_trans.copy_((t / t.sum(1, keepdim=True)).log().float())
            self.log_init.copy_((i / i.sum()).log().float())
            ev, _, _, _, tc, ic = self._run(score, seq_off, want)
        objs.append(self.objective(ev, c))
        vals = [float(v) for v in torch.stack(objs).cpu()]
        self.initial_objective = vals[0]
        return vals[1:]
