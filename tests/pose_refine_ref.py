"""The refinement loop of flow3d/validator.py:424-455 on the oracle (oracle.camera generator -> oracle.scene render), in fp64 or
fp32 on the CPU: the reference of tests/test_gpu_pose_refine.py, computed once per process and shared (not a test module).

The scene is tests/test_gpu_scene_model.py's: N = 300 (150 foreground), 64 x 48, four bases, a MoveModel with non-zero head biases,
so that the input-pose term of the MoveModel is live.  The target image is the oracle's fp64 render from the pose
[(I + d T_R) R0 | d T_t + t0], d = OFFSET_D, (T_R, T_t) = OFFSET_SIGNS: every one of the 12 parameters is off by the same d.

Why this offset and not a rotation of 0.02 rad.  The comparison needs a path on which no gradient component changes sign (Adam steps by
about lr x sign(g): a component whose gradient crosses zero turns round, and fp32 noise decides when).  (a) Under a pure rotation the three
diagonal entries of transR are off by O(angle^2): their gradients start near zero and flip within a few iterations - every rotation axis,
angle (0.02, 0.05) and translation tried left 1 - 8 of the 12 components changing sign.  (b) The splats of this scene are 1 - 2 pixels
wide, so an offset that moves them by pixels (0.02 x depth 2 .. 10 x fx 64 / depth) is beyond the range where the L1 loss is close to
linear in the pose; with d = 0.005 (sub-pixel) it is.  (c) Adam moves all 12 parameters at the same speed, so it walks in a straight line
towards a target that is off by the same d in every parameter, along sign(g0) - and OFFSET_SIGNS is a fixed point of tau -> -sign(g0(tau)),
found by iterating it from a seeded start: on that line the residuals only shrink, and the fp64 gradient stays within 5 % of its start.
LR makes the 30 steps cover about 60 % of d."""
from __future__ import annotations

import copy
import functools
import warnings

import torch

from deblur4dgs_amd.synth import make_scene
from oracle import camera as ocam
from oracle import scene as oscene

N, G, KB, W, H, SEED, T_FRAME = 300, 150, 4, 64, 48, 17, 2.0
ITERS, LR, ETA_MIN = 30, 2e-4, 2e-6
OFFSET_D, OFFSET_SIGNS = 0.005, (1, -1, -1, -1, -1, -1, 1, 1, -1, -1, -1, -1)  # transR row-major, then transT


def scene():
    """-> (make_scene dict in fp32, MoveModel state_dict with the non-trivial heads): what the device model is built from."""
    sc = make_scene(N, G, KB, 1, W, H, seed=SEED, dtype=torch.float32, T=8)
    sc["scales"] = sc["scales"] + 1.3
    return sc


@functools.lru_cache(maxsize=None)
def _cpu_model():
    from deblur4dgs_amd.scene_model import GaussianParams, MotionBases, SceneModel

    sc = scene()
    keys = ("means", "quats", "scales", "colors", "opacities")
    fg = GaussianParams(*[sc[k][:G].clone() for k in keys], motion_coefs=sc["motion_coefs"].clone())
    bg = GaussianParams(*[sc[k][G:].clone() for k in keys])
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(SEED)  # before the model exists: the MoveModel's own layers are initialised from the global generator
        model = SceneModel(sc["K"][None].clone(), sc["viewmat"][None].clone(), fg, MotionBases(sc["rots"].clone(), sc["transls"].clone()), bg)
        with torch.no_grad():  # non-trivial camera deltas and exposure half-widths (a zero-initialised head has no input-pose term)
            for head in (model.move_model.RT_head0, model.move_model.RT_head1):
                head[-1].bias.copy_(0.004 * torch.randn(6))
                head[-1].weight.copy_(0.02 * torch.randn(6, 64))
            model.move_model.time_params.copy_(torch.tensor([[0.5, 0.3, 0.45, 0.6, 0.2, 0.5, 0.7, 0.5]]))
    return model, sc


def build_model(dev):
    """A copy of the one seeded model, on `dev`, and its scene dict."""
    model, sc = _cpu_model()
    return copy.deepcopy(model).to(dev), sc


def offset_pose(w2c: torch.Tensor) -> torch.Tensor:
    """The pose the target image is rendered from (fp64)."""
    tau = OFFSET_D * torch.tensor(OFFSET_SIGNS, dtype=torch.float64)
    out = torch.eye(4, dtype=torch.float64)
    out[:3, :3] = (torch.eye(3, dtype=torch.float64) + tau[:9].reshape(3, 3)) @ w2c[:3, :3].double()
    out[:3, 3] = tau[9:] + w2c[:3, 3].double()
    return out


def _oracle_render(parts, sd, w2c, K):
    fg, bg, bases = parts
    RTs, times, _ = ocam.forward_start_end_mid(sd, w2c[:3, :3], w2c[:3, 3:4], T_FRAME, 11, "second")
    return oscene.render_exposure(fg, bg, bases, times[0, 5:6].to(w2c.dtype), RTs[5:6].to(w2c.dtype), w2c, K, (W, H), bg_color=1.0,
                                  return_depth=True, single=True)["img"]


def _leaves(dtype):
    model, sc = build_model("cpu")
    dd = lambda x: x.detach().to(dtype).clone()
    fg = {k: dd(v) for k, v in model.fg.params.items()}
    bg = {k: dd(v) for k, v in model.bg.params.items()}
    bases = {k: dd(v) for k, v in model.motion_bases.params.items()}
    sd = {k: dd(v) for k, v in model.move_model.state_dict().items()}
    return (fg, bg, bases), sd, sc["viewmat"].to(dtype), sc["K"].to(dtype)


@functools.lru_cache(maxsize=None)
def target_image() -> torch.Tensor:
    """[1,H,W,3] fp64: the oracle's render from the offset pose."""
    parts, sd, w2c, K = _leaves(torch.float64)
    with torch.no_grad():
        return _oracle_render(parts, sd, offset_pose(w2c), K)


@functools.lru_cache(maxsize=None)
def oracle_loop(dtype=torch.float64, iters: int = ITERS, lr: float = LR, eta_min: float = ETA_MIN) -> dict:
    """The reference's loop, literally -> dict(p [iters,12] after every update, losses [iters], grads [iters,12]) in fp64 tensors."""
    parts, sd, w2c, K = _leaves(dtype)
    img = target_image().to(dtype)
    transR = torch.nn.Parameter(torch.eye(3, dtype=dtype))
    transT = torch.nn.Parameter(torch.zeros(3, 1, dtype=dtype))
    opt = torch.optim.Adam([{"params": [transR, transT], "lr": lr}])
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=iters, eta_min=eta_min)
    ps, losses, grads = [], [], []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # scheduler.step() before optimizer.step(): the reference's order
        for _ in range(iters):
            w2c_trans = torch.zeros_like(w2c)
            w2c_trans[:3, :3] = transR @ w2c[:3, :3]
            w2c_trans[:3, 3:] = transT + w2c[:3, 3:]
            loss = (_oracle_render(parts, sd, w2c_trans, K) - img).abs().mean()
            loss.backward()
            grads.append(torch.cat([transR.grad.reshape(-1), transT.grad.reshape(-1)]).double().clone())
            sched.step()
            opt.step()
            opt.zero_grad(set_to_none=True)
            losses.append(loss.detach().double())
            ps.append(torch.cat([transR.detach().reshape(-1), transT.detach().reshape(-1)]).double().clone())
    return dict(p=torch.stack(ps), losses=torch.stack(losses), grads=torch.stack(grads))
