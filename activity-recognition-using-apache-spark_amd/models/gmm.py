"""GaussianMixture / GaussianMixtureModel — MLlib's ``GaussianMixture`` (EM, full covariances) with Spark's
parameter names plus ``covarianceType`` / ``regCovar`` / ``initMode``; ``har/ops/gmm.py`` defines every operation.

Engine: the rows are standardised once (``Z = (X - mean) / std``), then every iteration is ``gmm_estep``
(the Mahalanobis products on the fp32 matrix cores, the softmax epilogue, the moments about the old means
in per-workgroup slabs), ``gmm_finish`` (per component: fp64 slab sums, new mean, covariance, Cholesky
factor, ``W = L^{-T}`` and ``c``) and ``gmm_control`` (log-likelihood, history, converged flag, iteration
counter).  On a GPU a fit of ``maxIter`` iterations is therefore enqueued without any device -> host read;
once the converged flag is set the remaining launches leave the state untouched.  A final E-step under
the final parameters gives the log-likelihood, the training rows' clusters and the cluster sizes, which
are read once after the fit.  Nothing uses atomics, so a fit is bitwise reproducible.

Initialisation: ``"k-means"`` runs ``KMeans(k, maxIter=initSteps, seed)`` on the working rows and starts
from its centres, the cluster shares as weights and identity covariances; ``"random"`` takes the k rows
with the smallest Philox keys of ``STREAM_GMM_INIT`` as means, with equal weights.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np
import torch

from ..data.table import Column, Table
from ..ops import gmm as GM
from .base import Estimator, Model, features_tensor, new_uid, resolve_device
from .kmeans import KMeans, cluster_label_map


@dataclass
class GaussianMixtureSummary:
    logLikelihood: float = 0.0
    logLikelihoodHistory: List[float] = field(default_factory=list)
    clusterSizes: List[int] = field(default_factory=list)
    numIter: int = 0
    converged: bool = False
    k: int = 0
    predictions: Optional[torch.Tensor] = None   # int32 clusters of the training rows

    def as_dict(self):
        return {"logLikelihood": self.logLikelihood, "logLikelihoodHistory": list(self.logLikelihoodHistory),
                "clusterSizes": list(self.clusterSizes), "numIter": self.numIter, "converged": self.converged,
                "k": self.k}


class GaussianMixtureModel(Model):
    _param_names = ("featuresCol", "predictionCol", "probabilityCol")
    featuresCol = "features"
    predictionCol = "prediction"
    probabilityCol = "probability"

    def __init__(self, mu, W, weights, mean, std, summary: Optional[GaussianMixtureSummary] = None, uid=None,
                 device=None, label_map=None, c=None):
        """``mu`` [K, D], ``W`` [K, D, D] and ``c`` [K] are the working-coordinate operands (``c`` = None: rebuilt
        from ``W``'s diagonal and the weights), ``weights`` [K] fp64.  A fitted model carries the fit's own
        ``c``, so its predictions and scores are those of the fit's final E-step, bit for bit."""
        super().__init__(uid or new_uid("GaussianMixture"))
        self.device = torch.device(device) if device is not None else mu.device
        f32 = dict(device=self.device, dtype=torch.float32)
        self._mu = mu.to(**f32).contiguous()
        self._W = W.to(**f32).contiguous()
        self.weights = weights.to(device=self.device, dtype=torch.float64).contiguous()
        self.mean = mean.to(**f32).contiguous()
        self.std = std.to(**f32).contiguous()
        self._inv_std = (1.0 / self.std.double()).float()
        K, D = self._mu.shape
        GM.check_native_range(K, D)
        if c is None:   # sum log L_ii = -sum log W_ii: c from the stored operands alone
            logdet = -torch.log(torch.diagonal(self._W.double(), dim1=-2, dim2=-1)).sum(dim=1)
            c = GM.component_c(self.weights, logdet, D)
        self._c = c.to(**f32).contiguous()
        self._log_jac = float(torch.log(self.std.double()).sum())
        self.summary = summary or GaussianMixtureSummary(k=K)
        self.majority_labels = None if label_map is None else [int(v) for v in label_map]
        self.feature_cols = None   # the table columns the model was fitted on (None: the features column)

    @property
    def k(self) -> int:
        return int(self._mu.shape[0])

    @property
    def num_features(self) -> int:
        return int(self._mu.shape[1])

    def gaussians(self):
        """(means fp64 [K, D], covariances fp64 [K, D, D]) in the original coordinates."""
        sd = self.std.double()
        L = torch.linalg.inv(self._W.double()).transpose(-1, -2)      # W = L^-T
        Sigma = L @ L.transpose(-1, -2)
        return (self.mean.double().view(1, -1) + self._mu.double() * sd.view(1, -1),
                Sigma * sd.view(1, -1, 1) * sd.view(1, 1, -1))

    def _working_rows(self, X: torch.Tensor) -> torch.Tensor:
        X = X.to(device=self.device, dtype=torch.float32)
        if X.dim() != 2 or X.shape[1] != self.num_features:
            raise ValueError(f"GaussianMixtureModel takes [N, {self.num_features}] rows, got {tuple(X.shape)}")
        return GM.working_rows(X, self.mean, self._inv_std)

    def _estep(self, X: torch.Tensor, native: Optional[bool] = None) -> GM.EstepResult:
        Z = self._working_rows(X)
        if Z.shape[0] == 0:
            e = torch.zeros(0, dtype=torch.float32, device=self.device)
            return GM.EstepResult(resp=e.view(0, self.k), lse=e, pred=e.to(torch.int32))
        return GM.estep(Z, self._mu, self._W, self._c, None, native, want_moments=False)

    def predict(self, X: torch.Tensor, native: Optional[bool] = None) -> torch.Tensor:
        """int64 component of every row (the lowest index among equal responsibilities)."""
        return self._estep(X, native).pred.long()

    def predictProbability(self, X: torch.Tensor, native: Optional[bool] = None) -> torch.Tensor:
        return self._estep(X, native).resp

    def score_samples(self, X: torch.Tensor, native: Optional[bool] = None) -> torch.Tensor:
        """fp64 [N]: the log density of every row in the ORIGINAL coordinates (the working-coordinate
        value minus ``sum log std``, the Jacobian of the standardisation)."""
        return self._estep(X, native).lse.double() - self._log_jac

    def transform(self, table: Table) -> Table:
        e = self._estep(features_tensor(table, self.featuresCol, self.device))
        t = table.with_column(Column(self.probabilityCol, "vector", e.resp.double().cpu().numpy()))
        return t.with_column(Column(self.predictionCol, "double", e.pred.double().cpu().numpy(),
                                    meta={"nullable": False}))

    def label_map(self, pred: torch.Tensor, y: torch.Tensor, num_classes: int):
        """As ``KMeansModel.label_map``: (cluster x label table, majority label per cluster, purity)."""
        cm, majority, purity = cluster_label_map(self.k, self.device, pred, y, num_classes)
        self.majority_labels = [int(v) for v in majority.tolist()]
        return cm, majority, purity

    def state(self):
        s = self.summary
        out = {"mu": self._mu.cpu(), "W": self._W.cpu(), "c": self._c.cpu(), "weights": self.weights.cpu(), "mean": self.mean.cpu(),
               "std": self.std.cpu(),
               "loglik_history": torch.tensor(s.logLikelihoodHistory, dtype=torch.float64),
               "cluster_sizes": torch.tensor(s.clusterSizes, dtype=torch.int64),
               "loglik": torch.tensor([s.logLikelihood], dtype=torch.float64),
               "num_iter": torch.tensor([s.numIter, int(s.converged)], dtype=torch.int64)}
        if self.majority_labels is not None:
            out["majority_labels"] = torch.tensor(self.majority_labels, dtype=torch.int64)
        out["feature_cols"] = None if self.feature_cols is None else list(self.feature_cols)
        return out

    @classmethod
    def from_state(cls, st, uid=None, device=None) -> "GaussianMixtureModel":
        ni = st["num_iter"].tolist()
        summ = GaussianMixtureSummary(float(st["loglik"][0]), [float(v) for v in st["loglik_history"].tolist()],
                                      [int(v) for v in st["cluster_sizes"].tolist()], int(ni[0]), bool(ni[1]),
                                      int(st["mu"].shape[0]))
        lm = st["majority_labels"].tolist() if "majority_labels" in st else None
        return cls(st["mu"], st["W"], st["weights"], st["mean"], st["std"], summ, uid=uid, device=device, label_map=lm,
                   c=st.get("c"))

    def __str__(self):
        return f"GaussianMixtureModel (uid={self.uid}) with k={self.k}"


class GaussianMixture(Estimator):
    _param_names = ("k", "maxIter", "tol", "seed", "covarianceType", "regCovar", "initMode", "initSteps",
                    "featuresCol", "predictionCol", "probabilityCol", "weightCol", "device")

    def __init__(self, k: int = 2, maxIter: int = 100, tol: float = 0.01, seed: int = 0, covarianceType: str = "full",
                 regCovar: float = 1e-6, initMode: str = "k-means", initSteps: int = 5, featuresCol="features",
                 predictionCol="prediction", probabilityCol="probability", weightCol=None, device=None):
        super().__init__(new_uid("GaussianMixture"))
        self.k, self.maxIter, self.tol, self.seed = k, maxIter, tol, seed
        self.covarianceType, self.regCovar, self.initMode, self.initSteps = covarianceType, regCovar, initMode, initSteps
        self.featuresCol, self.predictionCol, self.probabilityCol = featuresCol, predictionCol, probabilityCol
        self.weightCol, self.device = weightCol, device

    def fit(self, table: Table) -> GaussianMixtureModel:
        dev = resolve_device(self.device)
        X = features_tensor(table, self.featuresCol, dev)
        w = None
        if self.weightCol is not None:
            w = torch.as_tensor(np.asarray(table[self.weightCol].data)).to(dev)
        model = self._fit_tensors(X, w)
        model.featuresCol, model.predictionCol, model.probabilityCol = (self.featuresCol, self.predictionCol,
                                                                        self.probabilityCol)
        return model

    def fit_tensors(self, X, weights=None) -> GaussianMixtureModel:
        return self._fit_tensors(X, weights)

    def _check(self, N: int, D: int):
        k = int(self.k)
        GM.check_native_range(k, D, N)
        if k > N:
            raise ValueError(f"GaussianMixture k = {k} exceeds the {N} rows")
        if int(self.maxIter) < 0 or float(self.tol) < 0.0 or float(self.regCovar) < 0.0 or int(self.initSteps) < 0:
            raise ValueError("maxIter, tol, regCovar and initSteps must be >= 0")
        if self.covarianceType not in ("full", "diag"):
            raise ValueError(f"covarianceType must be 'full' or 'diag', got {self.covarianceType!r}")
        if self.initMode not in ("k-means", "random"):
            raise ValueError(f"initMode must be 'k-means' or 'random', got {self.initMode!r}")

    def _init(self, Z: torch.Tensor, native: bool):
        """(means [k, D] working coordinates, weights fp64 [k])."""
        k, dev = int(self.k), Z.device
        if self.initMode == "random":
            rows = GM.random_init_rows(int(self.seed), k, Z.shape[0])
            return (Z.index_select(0, torch.from_numpy(rows).to(dev)).contiguous(),
                    torch.full((k,), 1.0 / k, dtype=torch.float64, device=dev))
        km = KMeans(k=k, maxIter=int(self.initSteps), seed=int(self.seed), device=dev)._fit_tensors(Z, native=native)
        sizes = torch.tensor(km.summary.clusterSizes, dtype=torch.float64, device=dev)
        return km.clusterCenters().to(dev).contiguous(), sizes / sizes.sum().clamp_min(1.0)

    def _fit_tensors(self, X, weights=None, native=None, initial_means=None, max_blocks: int = 0,
                     dtype=torch.float64) -> GaussianMixtureModel:
        """The fit.  Private knobs of the probe and the tests: ``native=False`` runs the PyTorch definitions on
        GPU tensors (``dtype``: the precision they evaluate the E-step in), ``initial_means`` [k, D] (original
        coordinates) replaces the initialisation (equal weights), ``max_blocks`` caps the E-step's grid."""
        if X.dim() != 2:
            raise ValueError("GaussianMixture takes a [N, D] matrix")
        N, D = X.shape
        self._check(N, D)
        dev = X.device
        native = X.is_cuda if native is None else bool(native)
        k, M = int(self.k), int(self.maxIter)
        reg, diag, tol = float(self.regCovar), self.covarianceType == "diag", float(self.tol)
        w = None
        if weights is not None:
            w = torch.as_tensor(weights).to(device=dev, dtype=torch.float32).contiguous()
            if w.numel() != N:
                raise ValueError("one weight per row")
        mean, std, inv_std = GM.standardizer(X.float())
        Z = GM.working_rows(X, mean, inv_std)
        if initial_means is not None:
            m0 = torch.as_tensor(initial_means).to(device=dev, dtype=torch.float32)
            if tuple(m0.shape) != (k, D):
                raise ValueError(f"initial_means must be [{k}, {D}]")
            mu0 = ((m0 - mean.view(1, D)) * inv_std.view(1, D)).contiguous()
            pi0 = torch.full((k,), 1.0 / k, dtype=torch.float64, device=dev)
        else:
            mu0, pi0 = self._init(Z, native)
        W0 = torch.eye(D, dtype=torch.float32, device=dev).expand(k, D, D).contiguous()
        c0 = GM.component_c(pi0, torch.zeros(k, dtype=torch.float64, device=dev), D)
        st = GM.FitState.alloc(mu0, W0, c0, pi0, M)

        if native:
            G = GM.grid(N, D, k, max_blocks)
            slabs = torch.empty(G, k, GM.slab_size(D), dtype=torch.float32, device=dev)
            part = torch.zeros(G, dtype=torch.float64, device=dev)
            for _ in range(M):
                GM.step_native(st, Z, w, reg, diag, tol, M, slabs, part, max_blocks)
            fin = GM.estep_native(Z, st.mu, st.W, st.c, w, want_moments=False, max_blocks=max_blocks)
        else:
            for _ in range(M):
                GM.step_torch(st, Z, w, reg, diag, tol, M, dtype)
            fin = GM.estep_torch(Z, st.mu, st.W, st.c, w, False, dtype)
        # ---- the fit's reads ----
        it, conv = (int(v) for v in st.state.tolist())
        hard = torch.bincount(fin.pred.long(), minlength=k).tolist()
        summ = GaussianMixtureSummary(float(fin.loglik), [float(v) for v in st.hist[:it].tolist()],
                                      [int(v) for v in hard], it, bool(conv), k, fin.pred)
        return GaussianMixtureModel(st.mu, st.W, st.pi, mean, std, summ, uid=self.uid, device=dev, c=st.c)


__all__ = ["GaussianMixture", "GaussianMixtureModel", "GaussianMixtureSummary"]
