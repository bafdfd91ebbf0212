"""HMMSmoother — an activity timeline from per-window class probabilities (new capability; the
reference labels every window on its own).

Consecutive windows of one recording are not independent: people keep doing an activity for a while.
``HMMSmoother.fit`` counts the label transitions between consecutive rows of the same sequence (a
sequence = a maximal run of consecutive rows with equal ``sequenceCol``, in row order; the whole table
when the column is absent), and ``HMMSmootherModel`` decodes any classifier's ``probability`` column with
the exact Viterbi of ``har.ops.hmm`` — on a GPU the chunked max-plus scan of ``csrc/kernels/hmm.hip``.

With ``stay=p`` no labels are needed: the transition matrix has p on the diagonal and (1 - p) / (K - 1)
elsewhere, start and class priors are uniform (``fit`` then only reads the number of classes).

``HMMSmootherModel.posterior`` gives the smoothed probability of every window instead of one hard path
(forward-backward, ``csrc/kernels/hmm_fb.hip`` on a GPU), and ``emIter > 0`` refines the transition matrix
and the start vector by Baum-Welch on the table's probability column alone (emissions and the class prior
stay fixed), so an unlabelled recording can fit its own smoother.
"""
from __future__ import annotations

import math
from typing import List, Optional, Tuple

import numpy as np
import torch

from ..data.table import Column, DeviceColumn, Table
from ..ops import hmm as H
from .base import Estimator, Model, labels_tensor, new_uid, num_label_classes, resolve_device

EMISSIONS = ("scaled", "posterior")
METHODS = ("viterbi", "posterior")
EM_FLOOR = math.exp(H.LOG_FLOOR)   # Baum-Welch floors its probabilities where the decoder floors its scores


def sequence_offsets(table: Table, col: Optional[str]) -> torch.Tensor:
    """int64 [S + 1] host offsets of the maximal runs of equal ``col`` values in row order ([0, N] when
    the table has no such column)."""
    n = table.count()
    if col is None or col not in table:
        return torch.tensor([0, n] if n else [0], dtype=torch.int64)
    return offsets_of_keys(table[col])


def offsets_of_keys(c: Column) -> torch.Tensor:
    n = len(c)
    if n == 0:
        return torch.tensor([0], dtype=torch.int64)
    if isinstance(c, DeviceColumn) and c.kind != "vector":
        v = c.tensor
        change = (v[1:] != v[:-1]).cpu()
    else:
        v = np.asarray(c.data)
        change = torch.from_numpy(np.asarray(v[1:] != v[:-1], dtype=bool))
    starts = torch.nonzero(change).squeeze(1) + 1
    return torch.cat([torch.zeros(1, dtype=torch.int64), starts.to(torch.int64), torch.tensor([n], dtype=torch.int64)])


class HMMSmootherModel(Model):
    _param_names = ("sequenceCol", "probabilityCol", "outputCol", "emission")

    def __init__(self, logA: torch.Tensor, logpi: torch.Tensor, prior: torch.Tensor, emission: str = "scaled",
                 sequenceCol: str = "USER", probabilityCol: str = "probability", outputCol: str = "smoothedPrediction",
                 uid=None, device=None):
        super().__init__(uid or new_uid("HMMSmoother"))
        if emission not in EMISSIONS:
            raise ValueError(f"unknown emission {emission!r} (scaled | posterior)")
        self.logA, self.logpi, self.prior = logA.double().cpu(), logpi.double().cpu(), prior.double().cpu()
        self.emission, self.sequenceCol, self.probabilityCol, self.outputCol = emission, sequenceCol, probabilityCol, outputCol
        self.num_classes = int(self.logpi.numel())
        self.device = resolve_device(device)
        # the decoder's integer scores, fixed once on the host so that every device decodes the same model
        self.qA, self.qpi = H.quantize_logprob(self.logA), H.quantize_logprob(self.logpi)
        # the same model in the probability domain (forward-backward), from the integer scores
        self.P, self.p0 = H.transition_probs(self.qA), H.start_probs(self.qpi)
        self.emIterations: int = 0
        self.objectiveHistory: List[float] = []
        self._dev = {}

    def _scores_on(self, dev: torch.device):
        key = str(dev)
        if key not in self._dev:
            self._dev[key] = (self.qA.to(dev), self.qpi.to(dev), self.prior.to(dev), self.P.to(dev), self.p0.to(dev))
        return self._dev[key]

    def emission_scores(self, prob: torch.Tensor) -> torch.Tensor:
        if prob.dim() != 2 or prob.shape[1] != self.num_classes:
            raise ValueError(f"probabilities must be [N, {self.num_classes}], got {tuple(prob.shape)}")
        return H.emission_scores(prob, self._scores_on(prob.device)[2], self.emission)

    def decode_scores(self, E: torch.Tensor, seq_offsets) -> Tuple[torch.Tensor, torch.Tensor]:
        qA, qpi = self._scores_on(E.device)[:2]
        return H.viterbi(E, qA, qpi, seq_offsets)

    def decode(self, prob: torch.Tensor, seq_offsets) -> Tuple[torch.Tensor, torch.Tensor]:
        """(path int32 [N], score int64 [S] in quanta of 2^-20) of class probabilities [N, K] on any
        device; ``seq_offsets`` int64 [S + 1] (a host tensor)."""
        return self.decode_scores(self.emission_scores(prob), seq_offsets)

    def posterior(self, prob: torch.Tensor, seq_offsets) -> Tuple[torch.Tensor, torch.Tensor]:
        """(gamma fp64 [N, K], loglik fp64 [S]) of class probabilities [N, K] on any device: the smoothed
        probability of every window given its whole sequence, and every sequence's log-likelihood under
        the emission scores."""
        E = self.emission_scores(prob)
        P, p0 = self._scores_on(E.device)[3:]
        gamma, loglik, _ = H.forward_backward(H.emission_likelihoods(E), P, p0, seq_offsets)
        return gamma, H.loglik_of_scores(loglik, E, seq_offsets)

    def transform(self, table: Table, method: str = "viterbi") -> Table:
        if method not in METHODS:
            raise ValueError(f"unknown method {method!r} (viterbi | posterior)")
        c = table[self.probabilityCol]
        prob = torch.as_tensor(np.ascontiguousarray(c.data, dtype=np.float64)).to(self.device)
        off = sequence_offsets(table, self.sequenceCol)
        if method == "posterior":
            gamma, _ = self.posterior(prob, off)
            pred = H._lowest_argmax(gamma, dim=1)[1] if gamma.numel() else torch.empty(0, dtype=torch.int64)
            table = table.with_column(Column("smoothedProbability", "vector", gamma.cpu().numpy()))
            return table.with_column(Column(self.outputCol, "double", pred.double().cpu().numpy(), meta={"nullable": False}))
        path, _ = self.decode(prob, off)
        return table.with_column(Column(self.outputCol, "double", path.double().cpu().numpy(), meta={"nullable": False}))

    def state(self):
        st = {"logA": self.logA, "logpi": self.logpi, "prior": self.prior, "emission": self.emission}
        if self.emIterations:
            st.update(emIterations=int(self.emIterations), objectiveHistory=[float(v) for v in self.objectiveHistory])
        return st

    def __str__(self):
        return f"HMMSmootherModel (uid={self.uid}) with {self.num_classes} states, {self.emission} emissions"


def _floored(p: torch.Tensor, dim: int) -> torch.Tensor:
    """Normalise along ``dim``, floor at ``EM_FLOOR`` and normalise again."""
    p = p / p.sum(dim=dim, keepdim=True)
    p = p.clamp_min(EM_FLOOR)
    return p / p.sum(dim=dim, keepdim=True)


def penalty(P: torch.Tensor, p0: torch.Tensor, smoothing: float) -> torch.Tensor:
    """``smoothing * (sum log P + sum log p0)``: the log-prior that the pseudo-counts stand for."""
    return float(smoothing) * (torch.log(P).sum() + torch.log(p0).sum())


def baum_welch_step(B: torch.Tensor, P: torch.Tensor, p0: torch.Tensor, seq_offsets, smoothing: float):
    """One EM iteration on any device: one ``forward_backward(..., want_xi=True)``, then
    ``P <- rownorm(xi + smoothing)`` and ``p0 <- norm(sum of gamma at the sequence starts + smoothing)``, both
    floored at e^-32 and renormalised.  Returns (P', p0', the summed log-likelihood of the OLD parameters as a
    0-d tensor on the device)."""
    gamma, loglik, xi = H.forward_backward(B, P, p0, seq_offsets, want_xi=True)
    starts = torch.as_tensor(seq_offsets)[:-1].to(B.device)
    lam = float(smoothing)
    return _floored(xi + lam, 1), _floored(gamma[starts].sum(0) + lam, 0), loglik.sum()


class HMMSmoother(Estimator):
    _param_names = ("sequenceCol", "labelCol", "probabilityCol", "smoothing", "emission", "stay", "numClasses", "device",
                    "emIter", "emTol")

    def __init__(self, sequenceCol: str = "USER", labelCol: str = "label", probabilityCol: str = "probability",
                 smoothing: float = 1.0, emission: str = "scaled", stay: Optional[float] = None,
                 numClasses: Optional[int] = None, device=None, emIter: int = 0, emTol: float = 1e-6):
        super().__init__(new_uid("HMMSmoother"))
        if emission not in EMISSIONS:
            raise ValueError(f"unknown emission {emission!r} (scaled | posterior)")
        if stay is not None and not 0.0 < float(stay) <= 1.0:
            raise ValueError(f"stay must be in (0, 1], got {stay}")
        if stay is None and smoothing <= 0:
            raise ValueError("smoothing must be positive (a zero count has no logarithm)")
        self.sequenceCol, self.labelCol, self.probabilityCol = sequenceCol, labelCol, probabilityCol
        if int(emIter) < 0 or emTol < 0:
            raise ValueError("emIter and emTol must not be negative")
        self.smoothing, self.emission, self.stay, self.numClasses, self.device = smoothing, emission, stay, numClasses, device
        self.emIter, self.emTol = int(emIter), float(emTol)

    def _model(self, A, pi, prior) -> HMMSmootherModel:
        m = HMMSmootherModel(torch.log(A), torch.log(pi), prior, self.emission, self.sequenceCol, self.probabilityCol,
                             device=self.device)
        m.uid = self.uid
        return m

    def fit_stay(self, K: int) -> HMMSmootherModel:
        """The label-free model: ``stay`` on the diagonal, uniform elsewhere."""
        if self.stay is None:
            raise ValueError("fit_stay needs stay=p")
        if not 1 <= K <= H.MAX_STATES:
            raise ValueError(f"the decoder takes 1..{H.MAX_STATES} states, got {K}")
        p = float(self.stay)
        if K == 1:
            A = torch.ones(1, 1, dtype=torch.float64)
        else:
            A = torch.full((K, K), (1.0 - p) / (K - 1), dtype=torch.float64)
            A.fill_diagonal_(p)
        u = torch.full((K,), 1.0 / K, dtype=torch.float64)
        return self._model(A, u, u.clone())

    def fit_labels(self, y: torch.Tensor, seq_offsets: torch.Tensor, K: int) -> HMMSmootherModel:
        """From int64 labels [N] in row order and the sequences' offsets (counting is ``bincount``)."""
        if not 1 <= K <= H.MAX_STATES:
            raise ValueError(f"the decoder takes 1..{H.MAX_STATES} states, got {K}")
        y = y.detach().cpu().long()
        n = y.numel()
        off = H._host_offsets(seq_offsets, n)
        lam = float(self.smoothing)
        is_start = torch.zeros(n, dtype=torch.bool)
        is_start[off[:-1]] = True
        inner = ~is_start[1:]                               # row t continues row t - 1's sequence
        pairs = (y[:-1] * K + y[1:])[inner]
        A = torch.bincount(pairs, minlength=K * K).double().view(K, K) + lam
        pi = torch.bincount(y[is_start], minlength=K).double() + lam
        prior = torch.bincount(y, minlength=K).double() + lam
        return self._model(A / A.sum(1, keepdim=True), pi / pi.sum(), prior / prior.sum())

    def fit_em(self, model: HMMSmootherModel, prob: torch.Tensor, seq_offsets) -> HMMSmootherModel:
        """At most ``emIter`` Baum-Welch iterations from ``model`` on class probabilities [N, K] (any device)
        and their sequences; emissions and the class prior stay fixed.  One scalar is read per iteration: the
        penalised objective ``loglik + smoothing * (sum log P + sum log p0)`` of the current parameters, and
        the loop ends when its relative improvement falls below ``emTol``.  ``objectiveHistory[i]`` is the
        objective before update i (one more entry when the tolerance ended the loop)."""
        if self.emIter <= 0 or prob.shape[0] == 0:
            return model
        off = H._host_offsets(seq_offsets, prob.shape[0])
        E = model.emission_scores(prob)
        B = H.emission_likelihoods(E)
        base = H.loglik_of_scores(torch.zeros(off.numel() - 1, dtype=torch.float64, device=E.device), E, off).sum()
        P, p0 = model._scores_on(E.device)[3:]
        hist: List[float] = []
        done = 0
        for _ in range(self.emIter):
            nP, np0, ll = baum_welch_step(B, P, p0, off, self.smoothing)
            hist.append(float(ll + base + penalty(P, p0, self.smoothing)))  # the iteration's one host read
            if len(hist) > 1 and hist[-1] - hist[-2] < self.emTol * abs(hist[-2]):
                break
            P, p0 = nP, np0
            done += 1
        out = HMMSmootherModel(torch.log(P), torch.log(p0), model.prior, model.emission, model.sequenceCol,
                               model.probabilityCol, model.outputCol, uid=model.uid, device=model.device)
        out.emIterations, out.objectiveHistory = done, hist
        return out

    def _refine(self, model: HMMSmootherModel, table: Table) -> HMMSmootherModel:
        if self.emIter <= 0:
            return model
        if self.probabilityCol not in table:
            raise ValueError(f"emIter > 0 needs the table's {self.probabilityCol!r} column")
        prob = torch.as_tensor(np.ascontiguousarray(table[self.probabilityCol].data, dtype=np.float64)).to(model.device)
        return self.fit_em(model, prob, sequence_offsets(table, self.sequenceCol))

    def fit(self, table: Table) -> HMMSmootherModel:
        return self._refine(self._fit_initial(table), table)

    def _fit_initial(self, table: Table) -> HMMSmootherModel:
        if self.stay is not None:
            K = self.numClasses
            if K is None:
                if self.labelCol in table:
                    K = num_label_classes(table, self.labelCol, torch.device("cpu"))
                elif self.probabilityCol in table:
                    K = int(np.asarray(table[self.probabilityCol].data).shape[1])
                else:
                    raise ValueError("stay=p: give numClasses, or a table with the label or probability column")
            return self.fit_stay(int(K))
        cpu = torch.device("cpu")
        y = labels_tensor(table, self.labelCol, cpu)
        K = int(self.numClasses or num_label_classes(table, self.labelCol, cpu))
        return self.fit_labels(y, sequence_offsets(table, self.sequenceCol), K)
