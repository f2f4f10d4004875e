"""Test-time pose refinement of a validation view on the device: `Validator.validate_imgs_with_optimization`
(reference flow3d/validator.py:400-456), the only path the reference's `run_testing.py` scores its frames through.

Per frame the reference runs 500 iterations of: compose w2c_trans = [transR R0 | transT + t0] from a free 3x3 `transR` and a 3x1
`transT`, `model.render(t, w2c_trans, K, img_wh, return_depth=True)` (mode "mid", stage "second"), L1 against the image, backward,
`CosineAnnealingLR.step()`, `Adam.step()`.  Here one iteration is

    SceneModel.render with `pose_only` set   the forward of the staged chain; its backward is d4gs_pose_bwd (the camera's gradients
                                             and nothing of size N) plus the MoveModel's input-pose term (d4gs_pose_encode_bwd)
    |pred - img|.mean(), backward            plain torch ops; only W.grad is produced (`backward(inputs=[W])`)
    d4gs_pose_step                           one one-wave launch: gradient through the composition, lr(step + 1), Adam, next W

with every piece of optimizer state - parameters, moments, step count, learning rate - in device memory, so the iteration is
captured ONCE in a HIP graph and replayed; the host does nothing per iteration but launch the graph.  DESIGN.md section 25.
There is no eager / CPU fallback: tensors must live on a ROCm device.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib as L
from . import engine

BETAS, EPS = (0.9, 0.999), 1e-8  # torch.optim.Adam's defaults: what the reference's optimizer runs with


class _PoseState:
    """p [12] (transR row-major, transT), Adam's m and v, the int32 step count and the composed matrix W [4,4] (a leaf that
    requires grad: what the render differentiates) - all on the device.  `snapshot()` / `restore()` copy the 37 numbers that define
    the trajectory, and W, which is a function of them that the step kernel has already evaluated."""

    def __init__(self, w2c: torch.Tensor):
        dev = w2c.device
        self.base = w2c.detach().to(torch.float32).reshape(4, 4).contiguous().clone()
        self.pmv = torch.zeros(36, dtype=torch.float32, device=dev)
        self.pmv[0:9:4] = 1.0  # transR = I, transT = 0
        self.p, self.m, self.v = self.pmv[0:12], self.pmv[12:24], self.pmv[24:36]
        self.step = torch.zeros(1, dtype=torch.int32, device=dev)
        self.lr = torch.zeros(1, dtype=torch.float32, device=dev)
        W = self.base.clone()
        W[3] = torch.tensor([0.0, 0.0, 0.0, 1.0], device=dev)  # what d4gs_pose_step writes there (include/d4gs.h)
        self.W = W.requires_grad_()

    def snapshot(self):
        return self.pmv.clone(), self.step.clone(), self.W.detach().clone()

    def restore(self, snap):
        with torch.no_grad():
            self.pmv.copy_(snap[0])
            self.step.copy_(snap[1])
            self.W.copy_(snap[2])


def pose_step(state: _PoseState, v_W: torch.Tensor, lr0: float, eta_min: float, t_max: int, betas=BETAS, eps: float = EPS):
    """d4gs_pose_step on `state`: consumes the gradient of the composed matrix, leaves the next composed matrix in state.W."""
    assert v_W.is_cuda and v_W.dtype == torch.float32 and v_W.numel() == 16 and v_W.is_contiguous()
    vp = L.vp
    L.check(L.lib().d4gs_pose_step(vp(state.base), vp(v_W), vp(state.p), vp(state.m), vp(state.v), vp(state.step), float(lr0),
                                   float(eta_min), int(t_max), float(betas[0]), float(betas[1]), float(eps), vp(state.lr),
                                   vp(state.W), L.stream_of(v_W)), "d4gs_pose_step")


def refine_pose(model, t, w2c, K, img, iters: int = 500, lr: float = 1e-2, eta_min: float = 1e-4, graph: bool = True,
                check_every: int = 50, pose_only: bool = True) -> dict:
    """Refine the pose of one view against `img` [H,W,3] (or [1,H,W,3]) -> dict(transR [3,3], transT [3,1], w2c [4,4] the refined
    matrix, img [1,H,W,3] the LAST iteration's render - the one the reference scores, rendered before the last update -,
    losses [iters] and lrs [iters] device tensors (written without a host wait), recaptures: how many times the graph's
    intersection lists overflowed and the step was captured again).

    graph=True: one warm-up iteration runs eagerly and is discarded (it sizes the intersection lists and loads every kernel), then
    one iteration is captured in a HIP graph inside `engine.GraphWatch.capturing()` and replayed.  A captured render keeps the list
    capacity of its capture while the pose, and with it the intersection count, moves: every `check_every` replays and at the end
    `GraphWatch.check()` looks at the counts the last replay left.  On an overflow the state goes back to the snapshot of the last
    check that passed, the graph is dropped and captured again at the capacity the check recorded, and the iterations since that
    snapshot are run again - an overflowed iteration never contributes to the result.  (A check reads the counts of the replay just
    before it; lists are captured with 25 % + 4096 entries of headroom over the count they were sized from.)
    graph=False: the same kernels launched eagerly, the same checks - the same bits.
    pose_only=False keeps the full leaf backward (d4gs_project_bwd) in the iteration: the measurement's comparison.
    `int(t)` is read on the host once, before the capture."""
    L.need_gpu(w2c, "deblur4dgs_amd.refine_pose", " (no CPU fallback)")
    dev = w2c.device
    t = t if isinstance(t, (int, float)) else float(t)  # one host read per frame, before anything is captured
    img = img.detach().to(torch.float32).reshape(1, *img.shape[-3:]).contiguous()
    H, Wd = img.shape[1:3]
    K1 = K.detach().to(torch.float32).reshape(1, 3, 3).contiguous()
    st = _PoseState(w2c)
    losses = torch.zeros(iters, dtype=torch.float32, device=dev)
    lrs = torch.zeros(iters, dtype=torch.float32, device=dev)
    last = {}

    def one():
        out = model.render(t, st.W[None], K1, (Wd, H), return_depth=True)
        pred = out["img"]
        loss = (pred - img).abs().mean()
        loss.backward(inputs=[st.W])  # W.grad alone: d4gs_pose_bwd's term + the MoveModel's input-pose term
        idx = st.step.to(torch.int64)
        losses.scatter_(0, idx, loss.detach().reshape(1))
        pose_step(st, st.W.grad, lr, eta_min, iters)
        lrs.scatter_(0, idx, st.lr)
        last["img"] = pred.detach()

    def eager():
        st.W.grad = None
        one()

    def capture():
        st.W.grad = None  # born inside the capture: the same buffer at every replay
        g, watch = torch.cuda.CUDAGraph(), engine.GraphWatch()
        with watch.capturing(), torch.cuda.graph(g, stream=torch.cuda.Stream()):
            one()
        return g, watch

    saved = (model.pose_only, model.deferred_size_check)
    model.pose_only, model.deferred_size_check = bool(pose_only), True
    recaptures, done, captured = 0, 0, None
    try:
        snap = st.snapshot()
        eager()  # the warm-up: sizes the lists, loads the kernels; discarded whether or not its lists fitted
        st.restore(snap)
        if not graph:
            _drain_deferred()
        while done < iters:
            n = min(max(int(check_every), 1), iters - done)
            try:
                if graph:
                    if captured is None:
                        captured = capture()
                        _drain_deferred()  # (the warm-up's record: its count may update the guess, not the captured capacity)
                    for _ in range(n):
                        captured[0].replay()
                    captured[1].replayed()
                    captured[1].check()
                else:
                    for _ in range(n):
                        eager()
                    engine.check_deferred()
            except RuntimeError as e:
                if "INVALID" not in str(e):
                    raise
                st.restore(snap)  # the engine has recorded the capacity the lists needed
                captured, recaptures = None, recaptures + 1
                if not graph:
                    _drain_deferred()
                continue
            done += n
            snap = st.snapshot()
        final_img = last["img"].clone()
    finally:
        model.pose_only, model.deferred_size_check = saved
        st.W.grad = None
    p = st.p.clone()
    return dict(transR=p[:9].view(3, 3), transT=p[9:].view(3, 1), w2c=st.W.detach().clone(), img=final_img, losses=losses, lrs=lrs,
                recaptures=recaptures, state=st)


def _drain_deferred():
    """Read every outstanding deferred list-size record; an overflow among them belongs to an iteration that was discarded."""
    try:
        engine.check_deferred()
    except RuntimeError as e:
        if "INVALID" not in str(e):
            raise


def validate_with_pose_refinement(model, frames, metrics=None, **refine_kw) -> dict:
    """The reference's validation loop (flow3d/validator.py:400-475) over `frames`: an iterable of dicts with `t`, `w2c` [4,4] or
    [1,4,4], `K`, `img` [H,W,3] or [1,H,W,3] and, optionally, `valid_mask` [H,W] (default: ones) and `fg_mask` [H,W] (default:
    zeros).  Each frame's pose is refined by `refine_pose(**refine_kw)`; the last iteration's render is scored by
    `metrics.ValidationMetrics` under the main, foreground and background masks, as the reference feeds its metrics.  Pass
    `metrics=ValidationMetrics(has_bg=model.has_bg, lpips=LPIPS(trunk, lins))` for the three LPIPS keys as well (deblur4dgs_amd.lpips).
    -> the reference's `val/*` keys (device scalars): six, or nine with `lpips=`."""
    from .metrics import ValidationMetrics

    metrics = ValidationMetrics(has_bg=model.has_bg) if metrics is None else metrics
    for f in frames:
        img = f["img"].reshape(1, *f["img"].shape[-3:])
        res = refine_pose(model, f["t"], f["w2c"], f["K"], img, **refine_kw)
        valid = f.get("valid_mask")
        valid = torch.ones_like(img[..., 0]) if valid is None else valid.reshape(img.shape[:-1]).float()
        fg = f.get("fg_mask")
        fg = torch.zeros_like(valid) if fg is None else fg.reshape(valid.shape).float()
        metrics.update(res["img"], img, valid, fg)
    return metrics.compute()
