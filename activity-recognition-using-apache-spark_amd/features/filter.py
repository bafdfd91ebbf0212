"""StreamFilter: Butterworth IIR conditioning of raw ``[S, A]`` streams before they are windowed.

The usual accelerometer recipe: a low-pass against sensor noise, and a 0.3 Hz low-pass whose output is "gravity"
and whose complement is "body acceleration".  ``ops.sosfilt`` holds the definition, the designer and the front-end
of the HIP kernels; a filter has nothing to fit, so the same object is the transform and what is saved::

    f = StreamFilter(hz=20, kind="split")                 # [body | gravity], 2A axes out
    z = f.transform(stream, seg_offsets)                  # fp32 [S, 6] of a 3-axis stream

Kinds
    ``lowpass``  low-pass at ``cutoff`` (default ``hz / 4``)
    ``gravity``  low-pass at ``cutoff`` (default 0.3 Hz)
    ``body``     ``x - gravity``
    ``split``    ``[x - gravity | gravity]``, 2A axes: feeds the window / spectral / rocket / DTW kernels as a 6-axis
                 stream of a 3-axis sensor
    ``sos``      the caller's own sections ``[sections, 6]``
``sos=`` with another kind replaces the designed low-pass branch by the caller's sections.

``zero_phase`` runs the filter forwards and backwards over every segment (no phase delay, squared magnitude);
``init`` is the state at a segment start (``step``: the steady state of the first sample's level, ``zero``).
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import torch

from ..ops import sosfilt as F

KINDS = ("lowpass", "gravity", "body", "split", "sos")
GRAVITY_HZ = 0.3
_MODE = {"lowpass": "filter", "gravity": "filter", "sos": "filter", "body": "body", "split": "split"}


class StreamFilter:
    def __init__(self, hz: float, kind: str = "lowpass", cutoff: Optional[float] = None, order: int = 3,
                 zero_phase: bool = False, sos=None, init: str = "step", uid: str = None):
        from ..models.base import new_uid

        if kind not in KINDS:
            raise ValueError(f"unknown filter kind {kind!r} ({' | '.join(KINDS)})")
        if init not in ("step", "zero"):
            raise ValueError(f"init must be 'step' or 'zero', got {init!r}")
        if zero_phase and init != "step":
            raise ValueError("the zero-phase form starts both passes from the step state")
        self.uid = uid or new_uid("StreamFilter")
        self.hz, self.kind, self.order = float(hz), kind, int(order)
        self.zero_phase, self.init = bool(zero_phase), init
        self.window_settings = None      # main.py: {"hz", "window_sec", "overlap"} of the run that saved the filter
        if sos is not None:  # the caller's sections: the whole filter of kind "sos", the low-pass branch of the others
            self.cutoff = None if cutoff is None else float(cutoff)
            self.sos = F._as_sos(sos)
        elif kind == "sos":
            raise ValueError("kind 'sos' needs the sections")
        else:
            self.cutoff = float(cutoff) if cutoff else (self.hz / 4.0 if kind == "lowpass" else GRAVITY_HZ)
            self.sos = F.butter_sos(self.order, self.cutoff, self.hz, "low")
        if F.power_growth(self.sos) > F.GUARD_BOUND:
            raise ValueError("the sections are too ill-conditioned for chunked evaluation (ops.sosfilt.check_range)")

    def __repr__(self) -> str:
        c = "" if self.cutoff is None else f", cutoff={self.cutoff:g} Hz"
        return (f"StreamFilter({self.kind}, hz={self.hz:g}{c}, sections={self.sos.shape[0]}"
                f"{', zero-phase' if self.zero_phase else ''})")

    @property
    def mode(self) -> str:
        return _MODE[self.kind]

    def out_axes(self, A: int) -> int:
        return 2 * int(A) if self.kind == "split" else int(A)

    def names(self, axis_names: Sequence[str] = ("X", "Y", "Z")) -> List[str]:
        """Output axis names: ``split`` gives ``BODY_*`` then ``GRAV_*``, ``body`` / ``gravity`` their prefix,
        the plain filters keep the input's names."""
        ax = list(axis_names)
        if self.kind == "split":
            return ["BODY_" + a for a in ax] + ["GRAV_" + a for a in ax]
        if self.kind == "body":
            return ["BODY_" + a for a in ax]
        if self.kind == "gravity":
            return ["GRAV_" + a for a in ax]
        return ax

    def transform(self, stream: torch.Tensor, seg_offsets=None) -> torch.Tensor:
        """fp32 [S, A] -> fp32 [S, out_axes(A)]; every run ``seg_offsets[i] .. seg_offsets[i + 1]`` on its own."""
        x = stream if stream.dtype == torch.float32 else stream.float()
        if self.zero_phase:
            return F.sosfiltfilt(x, self.sos, seg_offsets, self.mode)
        return F.sosfilt(x, self.sos, seg_offsets, self.init, False, self.mode)

    # ---- persistence (utils/persist.py) ----
    def params(self) -> dict:
        return {"hz": self.hz, "kind": self.kind, "cutoff": self.cutoff, "order": self.order,
                "zero_phase": self.zero_phase, "init": self.init}

    def state(self) -> dict:
        return {"sos": self.sos, "window_settings": self.window_settings}

    def to_state(self) -> dict:
        return {**self.params(), **self.state()}

    @classmethod
    def from_state(cls, tensors: dict, params: dict, uid: str = None, state: dict = None) -> "StreamFilter":
        """The saved sections are taken as they are (never re-designed): a reloaded filter has the same
        coefficient bits whatever the host's ``tan`` returns."""
        f = cls(params["hz"], params["kind"], params.get("cutoff"), int(params.get("order", 3)),
                bool(params.get("zero_phase", False)), tensors["sos"].double(), params.get("init", "step"), uid=uid)
        f.window_settings = (state or params).get("window_settings")
        return f
