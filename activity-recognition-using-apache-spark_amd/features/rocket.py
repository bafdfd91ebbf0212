"""RocketFeaturizer: MiniRocket-style convolutional window features of raw streams.

A fixed bank of 84 dilated 9-tap convolutions, pooled to one PPV number (the proportion of positive values)
per (kernel, dilation, bias); ``ops.rocket`` holds the definition, the float64 oracle and the front-end of the
HIP kernel.  ``fit`` only draws the axis subsets and reads the biases off example windows — there is no
back-propagation and no label — and is deterministic from the seed::

    model = RocketFeaturizer(hz=20, seconds=10, num_features=1680).fit(stream)    # stream [S, A]
    X = model.transform(stream)                                                    # fp32 [n_windows, F]
"""
from __future__ import annotations

from typing import List, Sequence

import torch

from ..ops.rocket import (RocketParams, _window_count, fit_rocket_params, rocket_features_into, rocket_features_torch,
                          rocket_names)


class RocketModel:
    """The fitted transform: window settings plus ``RocketParams``."""

    def __init__(self, params: RocketParams, hz: float, window: int, stride: int, seed: int = 0,
                 axis_names: Sequence[str] = ("X", "Y", "Z"), uid: str = None):
        from ..models.base import new_uid

        if params.window != window:
            raise ValueError("parameters and window settings disagree")
        self.uid = uid or new_uid("RocketModel")
        self.rocket_params, self.hz, self.window, self.stride, self.seed = params, float(hz), int(window), int(stride), int(seed)
        self.axis_names = list(axis_names)

    @property
    def num_features(self) -> int:
        return self.rocket_params.n_features

    @property
    def names(self) -> List[str]:
        return rocket_names(self.num_features)

    def halo(self) -> int:
        """Samples a shard must read past its end so no window straddling the cut is lost."""
        return max(0, self.window - self.stride)

    def transform_into(self, stream: torch.Tensor, out: torch.Tensor, col0: int = 0, stride: int = None) -> torch.Tensor:
        """Write the fp32 columns ``[col0, col0 + F)`` of the existing rows ``out`` (e.g. the tail of a
        ``[time | spectral | rocket]`` buffer).  ``stride`` overrides the model's window stride."""
        stride = self.stride if stride is None else int(stride)
        F = self.num_features
        if stream.is_cuda:
            rocket_features_into(stream if stream.dtype == torch.float32 else stream.float(), self.rocket_params,
                                 self.window, stride, out, col0)
            return out
        X = rocket_features_torch(stream, self.rocket_params, self.window, stride)
        if out.dim() != 2 or out.shape[0] != X.shape[0] or col0 < 0 or out.shape[1] < col0 + F:
            raise ValueError(f"out must be rows [{X.shape[0]}, >= {col0 + F}]")
        out[:, col0: col0 + F] = X.to(out.dtype)
        return out

    def transform(self, stream: torch.Tensor, stride: int = None) -> torch.Tensor:
        """[S, A] raw samples -> fp32 [n_windows, F]."""
        stride = self.stride if stride is None else int(stride)
        if not stream.is_cuda:
            return rocket_features_torch(stream, self.rocket_params, self.window, stride)
        out = torch.empty(_window_count(stream.shape[0], self.window, stride), self.num_features, dtype=torch.float32,
                          device=stream.device)
        return self.transform_into(stream, out, 0, stride)

    # ---- persistence (utils/persist.py) ----
    def params(self) -> dict:
        return {"hz": self.hz, "window": self.window, "stride": self.stride, "seed": self.seed,
                "axis_names": self.axis_names}

    def state(self) -> dict:
        p = self.rocket_params
        return {"masks": p.masks, "biases": p.biases, "axes": p.axes, "window": p.window}

    @classmethod
    def from_state(cls, tensors: dict, state: dict, params: dict, uid: str = None) -> "RocketModel":
        p = RocketParams(int(state["window"]), int(state["axes"]), tensors["masks"], tensors["biases"])
        return cls(p, params["hz"], params["window"], params["stride"], params.get("seed", 0),
                   params.get("axis_names", ("X", "Y", "Z")), uid=uid)


class RocketFeaturizer:
    """``fit(stream [S, A]) -> RocketModel`` with the WISDM window defaults (10 s at ``hz``; non-overlapping
    unless ``overlap`` > 0).  ``num_features`` is a target: the realised count is ``84 n_dil q`` with
    ``q = max(1, num_features // (84 n_dil))`` (1,680 at 200-sample windows)."""

    def __init__(self, hz: float = 20.0, seconds: float = 10.0, overlap: float = 0.0, num_features: int = 1680,
                 seed: int = 2018, axis_names: Sequence[str] = ("X", "Y", "Z")):
        self.hz = hz
        self.window = int(round(hz * seconds))
        self.stride = max(1, int(round(self.window * (1.0 - overlap))))
        self.num_features = int(num_features)
        self.seed = int(seed)
        self.axis_names = list(axis_names)

    def halo(self) -> int:
        return max(0, self.window - self.stride)

    def fit(self, stream: torch.Tensor) -> RocketModel:
        """Fit on the windows of ``stream`` at the featurizer's stride (features only, never labels)."""
        p = fit_rocket_params(stream, self.window, self.stride, self.num_features, self.seed)
        return RocketModel(p, self.hz, self.window, self.stride, self.seed, self.axis_names)
