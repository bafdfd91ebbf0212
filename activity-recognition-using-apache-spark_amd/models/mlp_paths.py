"""The native step paths of ``MLPEngine`` (models/mlp.py) and the holder of the fragment copies.  A path
owns what only it uses (loss / correct partials, private slabs, plans, streams) and answers ``takes``,
``forward_backward`` / ``run``, ``regions``, ``loss_and_correct`` and the constants of ``_Path``; the
engine builds those whose conditions hold, asks them in order and keeps the one that ran as ``last``."""
import os

import torch

from ..ops import _native
from ..ops.gemm import EPI_BIAS_RELU, EPI_F32_SLAB, EPI_RELU_GRAD, gemm_bf16

HEAD_PAD = 32  # classes padded to 32 rows (two 16-wide MFMA column tiles)


def n_splits_for(batch: int) -> int:
    """Batch slices of the split-K weight-gradient GEMMs (>= 1024-row slices, <= 64 slabs;
    ``HAR_MLP_SPLITS`` overrides the slab cap for tuning)."""
    cap = int(os.environ.get("HAR_MLP_SPLITS", "64"))
    return max(1, min(cap, batch // max(1, 65536 // cap)))


# Tile choices measured on MI355X with tools/gemm_bench.py (profiles/gemm_tile_sweep.md):
# ids index ops.gemm.TILES = (BM, BN, BK).
def fwd_tile(M: int, N: int, K: int) -> int:
    if K <= 64:
        return 12             # 64x128, BK 64
    return 6 if N >= 256 else 12  # 128x256 reads each activation row once


def dgrad_tile(M: int, N: int, K: int) -> int:
    return 18 if N >= 256 else 12    # 128x128 / 8 waves (24.0 us vs 24.8 for 128x256 at B = 65536)


def wgrad_tile(M: int, N: int) -> int:
    """Weight-gradient (split-K over the batch) tiles (profiles/gemm_tile_sweep_v2.md)."""
    if M <= 32:
        return 11 if N > 32 else 2   # 32x64, BK 128
    if N <= 64:
        return 20                    # 64x64, BK 128, 8 waves: 13.1 us vs 14.4 (4 waves)
    return 18                        # 128x128, BK 64, 8 waves: 23.4 us vs 30.0 (4 waves)


class FragCopies:
    """MFMA-fragment-ordered bf16 copies of W0 / W1 (W0 | W1 | W1^T; mlp.hip frag_pos): the step and small
    kernels load their weight operands from here, one 1 KB-contiguous load per fragment.  Owns ``Pf`` and
    whether it equals the weights.  The rule: a step on a path whose ``keeps_frag`` is False leaves the
    copies stale (the step forward writes W1^T from the pre-update W1, and Adam refreshes W0 | W1 only,
    and only on an engine with the step path: ``adam_args``); ``pack``, the GR_REFRESH kernel and the
    small path's Adam make them fresh.  Whoever reads all three calls ``ensure_fresh`` first."""

    def __init__(self, eng, on: bool, in_adam: bool):
        self.eng, self.Pf, self.fresh = eng, None, True
        self.args = self.adam_args = (0, 0, 0, 0, 0)  # (dst, W0 offset, W1 offset, K0, H); zeros: no copies
        if on:
            L, H = eng.layout, eng.layout.hidden[0]
            self.Pf = torch.zeros(H * L.in_pad + 2 * H * H, dtype=torch.bfloat16, device=eng.device)
            self.args = (self.Pf.data_ptr(), L.by_name["W0"].offset, L.by_name["W1"].offset, L.in_pad, H)
            if in_adam:
                self.adam_args = self.args
            self.pack()

    def pack(self):  # rebuild the copies from Pb
        if self.Pf is not None:
            _native.kernels().mlp_pack_frag(self.eng.Pb.data_ptr(), *self.args, _native.stream_ptr())
        self.fresh = True

    def mark_stale(self):
        self.fresh = False

    def ensure_fresh(self):
        if not self.fresh:
            self.pack()


class _Path:
    name = None
    fused = False       # forward + head are one kernel (MLPEngine.last_fused)
    ticks = False       # its backward kernel ticks the Adam step counter (else the reduction kernel does)
    keeps_frag = False  # a step on it leaves the fragment copies equal to the weights (FragCopies)
    whole_step = False  # one launch sequence is the whole step, Adam included: no forward_backward alone
    multiple = 1        # it takes batches of a multiple of this many rows

    def __init__(self, eng, nwg: int, max_batch: int):  # nwg: the most loss / correct partials (workgroups)
        self.e, self.nwg, self.max_batch = eng, nwg, max_batch
        self.loss = torch.zeros(nwg, dtype=torch.float32, device=eng.device)
        self.correct = torch.zeros(nwg, dtype=torch.int32, device=eng.device)

    def takes(self, Xb, yb) -> bool:  # (a well-formed batch: ``MLPEngine.select`` checks widths and types)
        return 0 < Xb.shape[0] <= self.max_batch and Xb.shape[0] % self.multiple == 0

    def run(self, Xb, yb, global_batch: int, adam: bool, prefetch=None):
        """forward + backward + the slab reduction, with Adam fused in (``adam``) or storing G."""
        e = self.e
        self.forward_backward(Xb, yb, 1.0 / global_batch)
        e._grad_kernel(e.GR_REDUCE | (e.GR_ADAM if adam else e.GR_STORE), tick=not self.ticks)

    def adam(self):  # Adam from the all-reduced G (the step counter ticked with the gradient)
        self.e.optimizer_step_native()

    def loss_and_correct(self):
        n = self.nwg
        return float(self.loss[:n].sum().item()), int(self.correct[:n].sum().item())

    def regions(self):  # its part of ``MLPEngine._grad_regions``; here: ``self.splits`` whole slabs
        e = self.e
        return [(0, e.layout.total, e.slabs.data_ptr(), self.splits, e.layout.total)]

    def _split_k(self, B: int) -> int:
        """k_split of the split-K weight-gradient GEMMs (a multiple of every BK); notes the slabs they fill."""
        n = self.e.n_splits
        ks = max(128, ((B + n - 1) // n + 127) // 128 * 128)
        self.splits = (B + ks - 1) // ks
        return ks

    def _wgrad(self, dact, act, name: str, M: int, N: int, B: int, ks: int, on_grad):
        """dW = dact^T . act (+ db = row sums of dact^T) into the slabs of W<name> / b<name>."""
        e, total = self.e, self.e.layout.total
        gemm_bf16(dact, act, e._slab("W" + name), M=M, N=N, K=B, layout=3, epi=EPI_F32_SLAB, k_split=ks, ldc=N,
                  slab_stride=total, rowsum=e._slab("b" + name), slab_stride_rowsum=total, tile=wgrad_tile(M, N))
        if on_grad is not None:
            on_grad("W" + name)


class GemmPath(_Path):
    """Any hidden layers: per-layer GEMMs, the fused head (head_fused), split-K weight-gradient GEMMs."""
    name = "gemm"

    def __init__(self, eng):
        super().__init__(eng, _native.kernels().head_fused_blocks(eng.B), eng.B)
        self.dlogits = torch.zeros(eng.B, HEAD_PAD, dtype=torch.bfloat16, device=eng.device)

    def forward_backward(self, Xb, y32, scale, on_grad=None, record=None):
        e, L, dims, B = self.e, self.e.layout, self.e.dims, Xb.shape[0]
        nh = len(L.hidden)
        if nh == 0:
            raise ValueError("the native MLP step needs at least one hidden layer")
        ks = self._split_k(B)
        acts = [Xb] + [a[:B] for a in e.acts[1:]]
        for i in range(nh):
            gemm_bf16(acts[i], e._w(e.Pb, f"W{i}"), acts[i + 1], M=B, N=dims[i + 1], K=dims[i], layout=0,
                      epi=EPI_BIAS_RELU, bias=e._w(e.P, f"b{i}"), tile=fwd_tile(B, dims[i + 1], dims[i]))
        last = acts[nh]
        # fused head: CE loss, dlogits, and dact of the last hidden layer = (dlogits . Wout) * relu'
        dact = e.dbuf[(nh - 1) % 2][: B * dims[-1]].view(B, dims[-1])
        _native.kernels().head_fused(
            last.data_ptr(), e._w(e.Pb, "Wout").data_ptr(), e._w(e.P, "bout").data_ptr(), y32.data_ptr(), B,
            dims[-1], L.num_classes, float(scale), self.dlogits.data_ptr(), dact.data_ptr(), self.loss.data_ptr(),
            self.correct.data_ptr(), _native.stream_ptr())
        self._wgrad(self.dlogits[:B], last, "out", HEAD_PAD, dims[-1], B, ks, on_grad)
        for i in reversed(range(nh)):
            h = dims[i + 1]
            self._wgrad(dact, acts[i], str(i), h, dims[i], B, ks, on_grad)
            if i > 0:
                # dact_{i-1} = (dact . W_i) * relu'(acts[i])
                hp = dims[i]
                prev = e.dbuf[(i - 1) % 2][: B * hp].view(B, hp)
                gemm_bf16(dact, e._w(e.Pb, f"W{i}"), prev, M=B, N=hp, K=h, layout=2, epi=EPI_RELU_GRAD,
                          mask=acts[i], tile=dgrad_tile(B, hp, h))
                dact = prev


class FusedFwdPath(_Path):
    """2-hidden-layer step of the shapes the three-kernel step does not take (H = 128, or a batch that
    is not a multiple of 64): ONE kernel for fwd L1 + fwd L2 + head + dWout/dbout (mlp_fused.hip; h2 and
    the logit gradients stay on chip; h1 and dact2 are written), then dW1, dgrad and dW0 as split-K MFMA
    GEMMs."""
    name, fused, multiple = "fused_fwd", True, 16

    def __init__(self, eng):
        nwg = _native.kernels().mlp_fwd_head_grid(eng.B)
        super().__init__(eng, nwg, eng.B)
        H = eng.layout.hidden[-1]  # per workgroup: dWout rows 0..15 [16][H], dbout [16] (+ an unused db1 slot)
        self.slab = torch.zeros(nwg, 16 * H + 16 + H, dtype=torch.float32, device=eng.device)
        # optional: the two backward branches after the fused forward — dW1 (split-K over the
        # batch) and dgrad -> dW0 — are independent, so HAR_MLP_STREAMS=1 runs dW1 on a second
        # HIP stream (fork/join with events; graph-capturable).  Measured on MI355X at batch
        # 65536: 0.147 vs 0.141 ms/step — both branches already fill every CU — so it is off.
        self.side = torch.cuda.Stream(eng.device) if os.environ.get("HAR_MLP_STREAMS", "0") == "1" else None
        self.ev_fork = torch.cuda.Event() if self.side is not None else None
        self.ev_join = torch.cuda.Event() if self.side is not None else None
        w = lambda t, n: eng._w(t, n).data_ptr()  # noqa: E731
        self.net = (eng.layout.in_pad, w(eng.Pb, "W0"), w(eng.P, "b0"), w(eng.Pb, "W1"), w(eng.P, "b1"), H,
                    w(eng.Pb, "Wout"), w(eng.P, "bout"))  # (mlp_fwd_head's K0 .. bo, fixed once)

    def forward_backward(self, Xb, y32, scale, on_grad=None, record=None):
        e, mod, s = self.e, _native.kernels(), _native.stream_ptr()
        B, H, K0 = Xb.shape[0], e.dims[-1], e.layout.in_pad
        ks = self._split_k(B)
        h1 = e.acts[1][:B]
        dact = e.dbuf[1][: B * H].view(B, H)
        self.nwg = mod.mlp_fwd_head_grid(B)

        def fwd():
            mod.mlp_fwd_head(Xb.data_ptr(), *self.net, y32.data_ptr(), B, e.layout.num_classes, float(scale),
                             h1.data_ptr(), dact.data_ptr(), self.slab.data_ptr(), self.loss.data_ptr(),
                             self.correct.data_ptr(), s)

        fwd()
        if record is not None:
            record.append(fwd)
        if on_grad is not None:
            on_grad("Wout")
        prev = e.dbuf[0][: B * H].view(B, H)
        main = torch.cuda.current_stream(e.device)
        if self.side is not None:  # fork: dW1 on the side stream, dgrad -> dW0 here
            self.ev_fork.record(main)
            self.side.wait_event(self.ev_fork)
            with torch.cuda.stream(self.side):
                self._wgrad(dact, h1, "1", H, H, B, ks, on_grad)
                self.ev_join.record(self.side)
        else:
            self._wgrad(dact, h1, "1", H, H, B, ks, on_grad)
        gemm_bf16(dact, e._w(e.Pb, "W1"), prev, M=B, N=H, K=H, layout=2, epi=EPI_RELU_GRAD, mask=h1,
                  tile=dgrad_tile(B, H, H))
        self._wgrad(prev, Xb, "0", H, K0, B, ks, on_grad)
        if self.side is not None:  # join: the W1 slabs (and the next step's h1 / dact2 reuse) are ordered
            main.wait_event(self.ev_join)

    def regions(self):
        """The split-K GEMM slabs up to Wout, then the forward's per-workgroup dWout / dbout slabs."""
        e, H, w, fs = self.e, self.e.dims[-1], self.slab.shape[1], self.slab.data_ptr()
        wo, bo = e.layout.by_name["Wout"].offset, e.layout.by_name["bout"].offset
        return [(0, wo, e.slabs.data_ptr(), self.splits, e.layout.total),
                (wo, wo + 16 * H, fs, self.nwg, w), (bo, bo + 16, fs + 4 * 16 * H, self.nwg, w)]


class StepPath(_Path):
    """The three-kernel step of the H = 256 network at batches % 64 (mlp_step.hip): mlp_step_fwd (layer 1,
    layer 2, softmax-CE head, dWout / dbout, and dact2 = (dz . Wout) * relu'(h2) in bf16), mlp_step_bwd (h1
    recomputed, dW1 + dgrad + relu' + dW0 / db0 / db1 in one pass), then the reduction + Adam.  A whole
    step goes through the native plan (bind.cpp MlpStepPlan) unless HAR_MLP_PLAN=0."""
    name, fused, ticks, multiple = "step", True, True, 64

    def __init__(self, eng):
        mod, dev = _native.kernels(), eng.device
        super().__init__(eng, mod.mlp_step_grid(eng.B), eng.B)
        self.slab = torch.zeros(self.nwg, mod.mlp_step_fwd_slab_width(256), dtype=torch.float32, device=dev)
        # the layer-2 gradient dact2 the forward writes for the backward (bf16 [B][256], the
        # backward's LDS tile order: 16-byte chunks of rows with bit 2 set swapped in pairs)
        self.dact2 = torch.zeros(eng.B * eng.layout.hidden[-1], dtype=torch.bfloat16, device=dev)
        self.pf_sink = torch.zeros(4, dtype=torch.int32, device=dev)  # scratch word of the prefetch workgroups
        self.use_plan = os.environ.get("HAR_MLP_PLAN", "1") != "0"
        self.plans = {}
        self.S = self.batch = 0  # row slices of the backward / rows of the last batch
        # every pointer and hyper-parameter of the step, fixed once (the fields of bind.cpp MlpStepPlan)
        e, L, P, Pb, sb = eng, eng.layout, eng.P, eng.Pb, eng.slabs.data_ptr()
        off = lambda n: sb + 4 * L.by_name[n].offset  # noqa: E731
        w = lambda t, n: e._w(t, n).data_ptr()  # noqa: E731
        self.d = dict(Wf=e.frag.Pf.data_ptr(), w0_off=L.by_name["W0"].offset, w1_off=L.by_name["W1"].offset,
                      b0=w(P, "b0"), b1=w(P, "b1"), Wo=w(Pb, "Wout"), bo=w(P, "bout"),
                      dact2=self.dact2.data_ptr(), fslab=self.slab.data_ptr(),
                      bloss=self.loss.data_ptr(), bcorr=self.correct.data_ptr(), gw1=off("W1"),
                      gw0=off("W0"), gb0=off("b0"), gb1=off("b1"), step=e.step_count.data_ptr(),
                      fslab_w=self.slab.shape[1], gwo=w(e.G, "Wout"), gbo=w(e.G, "bout"),
                      G=e.G.data_ptr(), P=P.data_ptr(), m=e.m.data_ptr(), v=e.v.data_ptr(), Pb=Pb.data_ptr(),
                      K0=L.in_pad, H=e.dims[-1], C=L.num_classes, stride=L.total, n=L.total, lr=float(e.lr),
                      beta1=float(e.betas[0]), beta2=float(e.betas[1]), eps=float(e.eps), wd=float(e.wd))

    def forward_backward(self, Xb, y32, scale, on_grad=None, record=None):  # record: one closure per kernel
        mod, d, B = _native.kernels(), self.d, Xb.shape[0]
        self.nwg, self.S, self.batch = mod.mlp_step_grid(B), mod.mlp_step_slices(B), B

        def fwd():
            mod.mlp_step_fwd(Xb.data_ptr(), d["K0"], d["Wf"], d["b0"], d["b1"], d["H"], d["Wo"], d["bo"],
                             y32.data_ptr(), B, d["C"], float(scale), d["dact2"], d["fslab"], d["bloss"], d["bcorr"],
                             _native.stream_ptr())

        def bwd():  # also sums the forward's dWout / dbout slabs into G
            mod.mlp_step_bwd(d["dact2"], Xb.data_ptr(), d["K0"], d["Wf"], d["H"], d["b0"], B, d["gw1"], d["gw0"],
                             d["gb0"], d["gb1"], d["stride"], d["step"], d["fslab"], d["fslab_w"], d["gwo"], d["gbo"],
                             _native.stream_ptr())

        fwd()
        if on_grad is not None:
            on_grad("Wout")
        bwd()
        if on_grad is not None:
            on_grad("W1")
            on_grad("W0")
        if record is not None:
            record += [fwd, bwd]

    def plan(self, B: int):
        """(MlpStepPlan, forward workgroups, backward row slices) at batch B: a step is ONE host call per
        phase.  Built on first use; building one runs nothing and leaves ``engine.last`` alone."""
        if B not in self.plans:
            mod = _native.kernels()
            nwg, S = mod.mlp_step_grid(B), mod.mlp_step_slices(B)
            plan = mod.MlpStepPlan(dict(self.d, regions=self.regions(S)))
            plan.pf_sink = self.pf_sink.data_ptr()
            self.plans[B] = (plan, nwg, S)
        return self.plans[B]

    def run(self, Xb, yb, global_batch: int, adam: bool, prefetch=None):
        """Plan modes: 1 reduce + Adam, 2 reduce + store G.  ``prefetch``: see MLPEngine.train_step."""
        if not self.use_plan:
            return super().run(Xb, yb, global_batch, adam)
        B = self.batch = Xb.shape[0]
        plan, self.nwg, self.S = self.plan(B)
        pf = []  # (pointer, bytes) of up to two regions; none: the plain launch
        for t in (prefetch if isinstance(prefetch, (tuple, list)) else (prefetch,)):
            if t is not None and t.is_cuda and t.numel():
                pf += [t.data_ptr(), t.numel() * t.element_size()]
        plan.run(Xb.data_ptr(), yb.data_ptr(), B, 1.0 / global_batch, 1 if adam else 2, _native.stream_ptr(), *pf)

    def adam(self):
        if not self.use_plan:
            return super().adam()
        self.plan(self.batch)[0].run(0, 0, self.batch, 0.0, 4, _native.stream_ptr())

    def regions(self, S=None):
        """The backward's partials (W0, b0, W1, b1) of S row slices; dWout / dbout: it summed them into G."""
        e, H = self.e, self.e.dims[-1]
        by, g = e.layout.by_name, e.G.data_ptr()
        w0, b1, wo, bo = by["W0"].offset, by["b1"].offset, by["Wout"].offset, by["bout"].offset
        return [(w0, b1 + H, e.slabs.data_ptr() + 4 * w0, self.S if S is None else S, e.layout.total),
                (wo, wo + 16 * H, g + 4 * wo, 1, 4), (bo, bo + 16, g + 4 * bo, 1, 4)]


class SmallPath(_Path):
    """Small batches (B <= 512, B % 32 == 0, one GPU): the whole forward + backward of each 32-row tile in
    one workgroup (mlp_small.hip) + the reduction / Adam of its B / 32 slabs — one host call, two
    launches per step.  Its Adam rewrites all three fragment copies."""
    name, ticks, keeps_frag, whole_step, multiple = "small", True, True, True, 32

    def __init__(self, eng):  # (the engine's capacity does not bound its batch: it uses no activations)
        n = _native.kernels().mlp_small_step_max_batch()
        super().__init__(eng, n // 32, n)
        e, L, step = eng, eng.layout, eng.step_count.data_ptr()
        w = lambda t, n: e._w(t, n).data_ptr()  # noqa: E731
        # mlp_small_step's arguments around the batch's own, fixed once (a step this small waits for the host)
        self.head = (L.in_pad, e.frag.Pf.data_ptr(), w(e.P, "b0"), w(e.P, "b1"), L.hidden[0], w(e.Pb, "Wout"),
                     w(e.P, "bout"))
        offs = (L.by_name[n].offset for n in ("W0", "b0", "W1", "b1", "Wout", "bout"))
        self.tail = (e.slabs.data_ptr(), L.total, *offs, self.loss.data_ptr(), self.correct.data_ptr(), step,
                     e.G.data_ptr(), e.P.data_ptr(), e.m.data_ptr(), e.v.data_ptr(), e.Pb.data_ptr(), float(e.lr),
                     *e.betas, float(e.eps), float(e.wd), step)

    def run(self, Xb, yb, global_batch: int, adam: bool = True, prefetch=None):
        B = Xb.shape[0]
        self.e.frag.ensure_fresh()  # a step of another path ran since: W1^T (and for H = 128 W0 / W1) re-packed
        self.nwg = self.splits = B // 32  # one loss / correct partial and one gradient slab per tile
        _native.kernels().mlp_small_step(Xb.data_ptr(), *self.head, yb.data_ptr(), B, self.e.layout.num_classes,
                                         1.0 / global_batch, *self.tail, _native.stream_ptr())
