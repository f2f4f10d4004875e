"""Seam S2: host-side mirror of the reference's scene model - same class names, `render()` signature, output dict
and side channels as flow3d/scene_model.py:162-487, flow3d/params.py:10-180 - with the whole device side of
`render()` replaced by ONE fused pass through libd4gs.so (deblur4dgs_amd.exposure.render_exposure).

What changes relative to the reference's render loop (scene_model.py:323-397):
  * the S exposure sub-samples are rendered by one deform+project launch and one composite launch instead of S
    iterations of ~60 torch launches + one gsplat call each;
  * activations (params.py:39-43) run inside the kernels on the raw leaves;
  * the per-sub-sample debug `cv2.imwrite` to a hard-coded path (scene_model.py:375-378) is NOT reproduced.
Reproduced quirks: camera delta moves means but not rotations (:352-353); blend channel 3 <- max, 16 <- min taken
after the in-place mean write, so `exposure_imgs[-1]` is the blended frame (:386-397, 486); `means`, `quats`,
`epoch` arguments are accepted and ignored (:174-175,183).
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from .engine import track_points
from .exposure import render_exposure
from .move_model import MoveModel

BLUR_NUM_CAMERAS = 11  # scene_model.py:248


class GaussianParams(nn.Module):
    """flow3d/params.py:10-118: raw leaves in a ParameterDict; same state_dict keys (`params.means`, ...)."""

    def __init__(self, means, quats, scales, colors, opacities, motion_coefs=None, scene_center=None, scene_scale=1.0):
        super().__init__()
        d = means.shape[:-1]
        assert quats.shape == (*d, 4) and scales.shape == (*d, 3) and colors.shape == (*d, 3) and opacities.shape == d
        p = {"means": nn.Parameter(means), "quats": nn.Parameter(quats), "scales": nn.Parameter(scales),
             "colors": nn.Parameter(colors), "opacities": nn.Parameter(opacities)}
        if motion_coefs is not None:
            assert motion_coefs.shape[:-1] == d
            p["motion_coefs"] = nn.Parameter(motion_coefs)
        self.params = nn.ParameterDict(p)
        self.register_buffer("scene_center", torch.zeros(3, device=means.device) if scene_center is None else scene_center)
        self.register_buffer("scene_scale", torch.as_tensor(scene_scale))

    @staticmethod
    def init_from_state_dict(state_dict, prefix="params."):
        req = ["means", "quats", "scales", "colors", "opacities"]
        assert all(f"{prefix}{k}" in state_dict for k in req)
        args = {"motion_coefs": None, "scene_center": torch.zeros(3), "scene_scale": torch.tensor(1.0)}
        for k in req + list(args):
            if f"{prefix}{k}" in state_dict:
                args[k] = state_dict[f"{prefix}{k}"]
        return GaussianParams(**args)

    @property
    def num_gaussians(self) -> int:
        return self.params["means"].shape[0]

    # activations (kept for callers that want the activated values; render() feeds the RAW leaves to the kernels)
    def get_colors(self):
        return torch.sigmoid(self.params["colors"])

    def get_scales(self):
        return torch.exp(self.params["scales"])

    def get_opacities(self):
        return torch.sigmoid(self.params["opacities"])

    def get_quats(self):
        return F.normalize(self.params["quats"], dim=-1, p=2)

    def get_coefs(self):
        return F.softmax(self.params["motion_coefs"], dim=-1)


    # ---- adaptive control (flow3d/params.py:86-118): the model side of densify / cull / reset ----------------
    def densify_params(self, should_split, should_dup, plan=None):
        """Row surgery on every parameter: kept rows (not split), then the duplicated rows, then every split row twice
        (the two halves of a split get scales / 1.6, i.e. log-scale - log 1.6).  Returns {name: new Parameter}.
        One RowPlan (stream compaction on the device) serves all parameters; pass `plan` to share it with the Adam
        state / statistics surgery of the same step."""
        from .rows import SPLIT_LOG_SCALE, RowPlan

        plan = plan or RowPlan(should_split, should_dup)
        out = {}
        for name in list(self.params.keys()):
            out[name] = nn.Parameter(plan.gather(self.params[name].detach(),
                                                 split_add=SPLIT_LOG_SCALE if name == "scales" else None))
            self.params[name] = out[name]
        return out

    def cull_params(self, should_cull, plan=None):
        from .rows import RowPlan

        plan = plan or RowPlan(should_cull)
        out = {}
        for name in list(self.params.keys()):
            out[name] = nn.Parameter(plan.gather(self.params[name].detach()))
            self.params[name] = out[name]
        return out

    def reset_opacities(self, new_val):
        self.params["opacities"].data.fill_(float(new_val))
        return {"opacities": self.params["opacities"]}

    def reorder_params(self, plan):
        """Rows permuted by `plan` (rows.RowPlan.from_permutation): the set of Gaussians is unchanged, only their order in
        memory (control.spatial_order_step).  Returns {name: new Parameter}."""
        out = {}
        for name in list(self.params.keys()):
            out[name] = nn.Parameter(plan.gather(self.params[name].detach()))
            self.params[name] = out[name]
        return out


class MotionBases(nn.Module):
    """flow3d/params.py:121-180: `rots [K,T,6]`, `transls [K,T,3]`."""

    def __init__(self, rots, transls):
        super().__init__()
        assert rots.shape[-1] == 6 and transls.shape[-1] == 3 and rots.shape[:-1] == transls.shape[:-1]
        self.num_frames, self.num_bases = rots.shape[1], rots.shape[0]
        self.params = nn.ParameterDict({"rots": nn.Parameter(rots), "transls": nn.Parameter(transls)})

    @staticmethod
    def init_from_state_dict(state_dict, prefix="params."):
        return MotionBases(state_dict[f"{prefix}rots"], state_dict[f"{prefix}transls"])

    def compute_transforms(self, ts: torch.Tensor, coefs: torch.Tensor) -> torch.Tensor:
        """(G,B,3,4) transforms at times ts (B,) for ACTIVATED coefficients `coefs` (G,K): flow3d/params.py:142-180 on
        the HIP path (d4gs_poses_fwd/bwd with D4GS_RAW_PARAMS clear: the coefficients are used as given)."""
        return _transforms(self, ts, coefs, raw=False)


def _ts1d(ts: torch.Tensor) -> torch.Tensor:
    """(B,) float32 times; the reference also accepts (1,B) (params.py:150-151) and integer frame indices."""
    ts = ts.reshape(-1) if ts.dim() == 2 and ts.shape[0] == 1 else ts
    assert ts.dim() == 1, "ts must be (B,) or (1,B)"
    return ts.to(torch.float32)


def _transforms(bases: "MotionBases", ts, coefs, raw: bool):
    from .engine import poses

    return poses(coefs.new_zeros(coefs.shape[0], 3), None, coefs, bases.params["rots"], bases.params["transls"], _ts1d(ts),
                 want=(False, False, True), raw_coefs=raw)[2]


class SceneModel(nn.Module):
    def __init__(self, Ks, w2cs, fg_params: GaussianParams, motion_bases: MotionBases, bg_params: GaussianParams | None = None):
        super().__init__()
        self.num_frames = motion_bases.num_frames
        self.fg, self.motion_bases, self.bg = fg_params, motion_bases, bg_params
        self.register_buffer("bg_scene_scale", torch.as_tensor(1.0 if bg_params is None else bg_params.scene_scale))
        self.register_buffer("Ks", Ks)
        self.register_buffer("w2cs", w2cs)
        self._current_xys = self._current_radii = self._current_img_wh = None
        self.move_model = MoveModel(num_fg=self.num_fg_gaussians, camera_mode="linear").to(Ks.device)
        self.inplace_blend_quirk = True  # exposure_imgs[-1] is the blended frame (scene_model.py:391,486)
        self._stats_sink = None
        self.fused = True  # one autograd node over d4gs_forward / d4gs_backward where the channel count allows it (same bits
        #                    as the staged chain, a fraction of the host work); False: always the staged chain
        self.deferred_size_check = False  # True: renders never wait for the device-side intersection count (engine
        #                                   RenderCfg.deferred_size_check; call engine.check_deferred() once per step)
        self.pose_only = False  # True: the scene is frozen and a backward differentiates only the camera - `w2cs` and, through the camera
        #                         deltas, the MoveModel (engine RenderCfg.pose_only; pose_refine.refine_pose sets it for its own renders)

    def attach_control_stats(self, running_stats: dict, batch_size: int, update_max_radii: bool = False, absgrad: bool = False):
        """SURVEY 8f-1, fused: until `detach_control_stats()`, the backward of every full render (all Gaussians, no
        filter mask) adds this step's densification statistics to `running_stats` inside the rasterizer's gather
        epilogue - what `Trainer._prepare_control_step` (flow3d/trainer.py:953-990) computes from
        `_current_xys[i].grad` / `_current_radii` after the step, without the S x 10 torch launches or the extra pass.
        `batch_size` = number of render groups of the step (trainer.py:965).
        absgrad=True: the grow criterion of gsplat's `DefaultStrategy(absgrad=True)` - the statistics accumulate the norm of
        absgrad (per pixel |dL/dx|, |dL/dy|, summed) instead of the gradient's, and after a backward `_current_xys[i].absgrad`
        holds it.  Renders of more than 16 colour channels cannot compute absgrad (NotImplementedError)."""
        self._stats_sink = (running_stats, int(batch_size), bool(update_max_radii), bool(absgrad))  # the dict itself: control
        #                                                                  steps replace its tensors when N changes

    def detach_control_stats(self):
        self._stats_sink = None

    def _sink_for(self, N: int):
        if self._stats_sink is None or not torch.is_grad_enabled():
            return None
        stats, batch_size, upd, absgrad = self._stats_sink
        if stats["vis_count"].shape[0] != N:
            return None
        return dict(stats, batch_size=batch_size, update_max_radii=upd, absgrad=absgrad)

    num_gaussians = property(lambda self: self.num_bg_gaussians + self.num_fg_gaussians)
    num_bg_gaussians = property(lambda self: self.bg.num_gaussians if self.bg is not None else 0)
    num_fg_gaussians = property(lambda self: self.fg.num_gaussians)
    num_motion_bases = property(lambda self: self.motion_bases.num_bases)
    has_bg = property(lambda self: self.bg is not None)

    def _all(self, getter: str) -> torch.Tensor:  # scene_model.py:122-143: fg rows first, then bg
        parts = [getattr(self.fg, getter)()] + ([getattr(self.bg, getter)()] if self.bg is not None else [])
        return parts[0] if len(parts) == 1 else torch.cat(parts, 0)

    def get_colors_all(self) -> torch.Tensor:
        return self._all("get_colors")

    def get_scales_all(self) -> torch.Tensor:
        return self._all("get_scales")

    def get_opacities_all(self) -> torch.Tensor:
        return self._all("get_opacities")

    @staticmethod
    def init_from_state_dict(state_dict, prefix=""):
        fg = GaussianParams.init_from_state_dict(state_dict, prefix=f"{prefix}fg.params.")
        bg = None
        if any("bg." in k for k in state_dict):
            bg = GaussianParams.init_from_state_dict(state_dict, prefix=f"{prefix}bg.params.")
        mb = MotionBases.init_from_state_dict(state_dict, prefix=f"{prefix}motion_bases.params.")
        return SceneModel(state_dict[f"{prefix}Ks"], state_dict[f"{prefix}w2cs"], fg, mb, bg)

    # ---- a4 / a5: the pose API the reference's Trainer / Renderer call on the model (flow3d/trainer.py:303,478,485,701,818;
    # flow3d/renderer.py:37), reference flow3d/scene_model.py:58-120, on the HIP path (engine.PosesFn) ----
    def compute_poses_bg(self) -> tuple[torch.Tensor, torch.Tensor]:
        """-> means (G_bg,3), quats (G_bg,4) (scene_model.py:58-65)."""
        assert self.bg is not None
        m, q = self._poses(self.bg.params["means"], self.bg.params["quats"], None, None)
        return m[:, 0], q[:, 0]

    def compute_transforms(self, ts: torch.Tensor, inds: torch.Tensor | None = None) -> torch.Tensor:
        """-> (G,B,3,4) (scene_model.py:67-74)."""
        coefs = self.fg.params["motion_coefs"]
        if inds is not None:
            coefs = coefs[inds]  # softmax is row-wise: softmax(c)[inds] == softmax(c[inds])
        return _transforms(self.motion_bases, ts, coefs, raw=True)

    def _poses(self, means, quats, coefs, ts):
        """means (n,B,3), quats (n,B,4): the first len(coefs) rows deformed to the times ts; ts None = the canonical
        pose (B = 1; means as given, quats normalised)."""
        from .engine import poses

        if ts is None:
            coefs, ts = None, means.new_zeros(1)
        mb = self.motion_bases.params
        m, q, _ = poses(means, quats, coefs, mb["rots"] if coefs is not None else None,
                        mb["transls"] if coefs is not None else None, _ts1d(ts))
        return m, q

    def compute_poses_fg(self, ts: torch.Tensor | None, inds: torch.Tensor | None = None) -> tuple[torch.Tensor, torch.Tensor]:
        """-> means (G,B,3), quats (G,B,4) wxyz (scene_model.py:76-106)."""
        means, quats, coefs = self.fg.params["means"], self.fg.params["quats"], self.fg.params["motion_coefs"]
        if inds is not None:
            means, quats, coefs = means[inds], quats[inds], coefs[inds]
        return self._poses(means, quats, coefs, ts)

    def compute_poses_all(self, ts: torch.Tensor | None) -> tuple[torch.Tensor, torch.Tensor]:
        """-> means (N,B,3), quats (N,B,4): fg rows deformed, bg rows repeated (scene_model.py:108-120).  One launch over
        the concatenated raw leaves (the static rows pass through the same kernel)."""
        P = self._raw("all")
        return self._poses(P["means"], P["quats"], self.fg.params["motion_coefs"], ts)

    def _raw(self, which: str):
        sets = {"fg": [self.fg], "bg": [self.bg], "all": [self.fg] + ([self.bg] if self.bg is not None else [])}[which]
        cat = lambda k: sets[0].params[k] if len(sets) == 1 else torch.cat([s.params[k] for s in sets], 0)
        return {k: cat(k) for k in ("means", "quats", "scales", "opacities", "colors")}

    def render(
        self,
        t,  # frame index / time (int | float | 1-element tensor | None)
        w2cs: torch.Tensor,  # (1,4,4)
        Ks: torch.Tensor,  # (1,3,3)
        img_wh: tuple[int, int],
        target_ts: torch.Tensor | None = None,  # (B,)
        target_w2cs: torch.Tensor | None = None,  # (B,4,4)
        bg_color: torch.Tensor | float = 1.0,
        colors_override: torch.Tensor | None = None,
        means: torch.Tensor | None = None,  # ignored (as in the reference)
        quats: torch.Tensor | None = None,  # ignored
        target_means: torch.Tensor | None = None,
        return_color: bool = True,
        return_depth: bool = False,
        return_mask: bool = False,
        fg_only: bool = False,
        bg_only: bool = False,
        filter_mask: torch.Tensor | None = None,
        epoch=1,  # ignored
        mode="mid",
        stage="second",
    ) -> dict:
        assert not (fg_only and bg_only)
        assert w2cs.shape[0] == 1, "C must be 1 (scene_model.py:249)"
        device = w2cs.device
        W, H = img_wh
        which = "fg" if fg_only else ("bg" if bg_only else "all")
        if which == "bg":
            assert self.bg is not None
        P = self._raw(which)
        N = P["means"].shape[0]
        G = 0 if which == "bg" or t is None else self.num_fg_gaussians
        n_sigmoid = 0
        if colors_override is None:
            if return_color:
                colors_override, n_sigmoid = P["colors"], 3
            else:
                colors_override = torch.zeros(N, 0, device=device)
        D = colors_override.shape[-1]
        if isinstance(bg_color, float):
            bg_color = torch.full((1, D), bg_color, device=device)
        ds_expected = {"img": D}
        if return_mask:  # :235-246
            mask_values = torch.ones(N, 1, device=device)
            if which == "all":
                mask_values[self.num_fg_gaussians:] = 0.0
            colors_override = torch.cat([colors_override, mask_values], -1)
            bg_color = torch.cat([bg_color, torch.zeros(1, 1, device=device)], -1)
            ds_expected["mask"] = 1

        # host-side generator: camera deltas + exposure times (a12)
        RTs, times, deltaT = self.move_model.forward_start_end_mid(
            info={"R": w2cs[0, :3, :3], "T": w2cs[0, :3, 3:4], "timestep": t if t is not None else 0.0},
            num_cameras=BLUR_NUM_CAMERAS, mode="uniform", stage=stage)

        B = 0
        if target_ts is not None:  # :258-289
            B = target_ts.shape[0]
            if target_means is None:  # fused HIP path: deform at the B target times + express in the target cameras
                tG = 0 if which == "bg" else self.num_fg_gaussians
                target_means = track_points(
                    P["means"], self.fg.params["motion_coefs"] if tG > 0 else None,
                    self.motion_bases.params["rots"] if tG > 0 else None,
                    self.motion_bases.params["transls"] if tG > 0 else None, target_ts.to(torch.float32), target_w2cs)
            elif target_w2cs is not None:
                target_means = torch.einsum("bij,pbj->pbi", target_w2cs[:, :3], F.pad(target_means, (0, 1), value=1.0))
            colors_override = torch.cat([colors_override, target_means.flatten(-2)], -1)
            bg_color = torch.cat([bg_color, torch.zeros(1, 3 * B, device=device)], -1)
            ds_expected["tracks_3d"] = 3 * B
        if return_depth:
            ds_expected["depth"] = 1

        sel = {"mid": slice(BLUR_NUM_CAMERAS // 2, BLUR_NUM_CAMERAS // 2 + 1), "start": slice(0, 1),
               "end": slice(BLUR_NUM_CAMERAS - 1, BLUR_NUM_CAMERAS)}.get(mode, slice(None))
        RTs_s, times_s = RTs[sel, :3, :], times[0, sel]
        S = RTs_s.shape[0]

        coefs = self.fg.params["motion_coefs"] if G > 0 else None
        if filter_mask is not None:  # :298-302, 355-358
            assert filter_mask.shape == (N,)
            P = {k: v[filter_mask] for k, v in P.items()}
            colors_override = colors_override[filter_mask]
            if G > 0:
                coefs = coefs[filter_mask[:G]]
                G = int(coefs.shape[0])
                if G == 0:
                    coefs = None
            N = P["means"].shape[0]

        # Any channel count (B target frames -> 3 + mask + 3B + depth): the engine composites wide colour vectors in
        # chunks of <= 16 channels over one projection / one set of sorted tile lists and returns exactly these
        # channels, so the reference's channel-index blend policy (3 <- max, 16 <- min, scene_model.py:392-393)
        # is evaluated on the reference's own layout.
        res = render_exposure(
            P["means"], P["quats"], P["scales"], P["opacities"], colors_override, n_sigmoid, coefs,
            self.motion_bases.params["rots"] if G > 0 else None, self.motion_bases.params["transls"] if G > 0 else None,
            times_s if G > 0 else None, RTs_s, w2cs[0], Ks[0], W, H, background=bg_color[0], return_depth=return_depth,
            policy=None, blend=True,
            control_stats=self._sink_for(N) if (which == "all" and filter_mask is None) else None,
            deferred_size_check=self.deferred_size_check, fused=self.fused, pose_only=self.pose_only,
            absgrad=self._stats_sink is not None and self._stats_sink[3] and torch.is_grad_enabled())
        blended = res["blended"][None]  # [1,H,W,D']
        renders = res["renders"]

        # side channels for densification (scene_model.py:456-461; consumed at trainer.py:967-989)
        m2d = res["means2d"]
        one_call = bool(res["state"].frame_io)  # engine.FrameFn: one autograd node, means2d is not an intermediate
        if m2d.requires_grad or (one_call and torch.is_grad_enabled() and blended.requires_grad):
            xys = [m2d.detach()[s:s + 1].requires_grad_() for s in range(S)]
            if one_call:
                res["state"].xys_sink = xys  # the backward deposits d loss / d means2d there
            else:
                def _deposit(g, xys=xys, st=res["state"]):
                    for s, x in enumerate(xys):
                        x.grad = g[s:s + 1]
                        if st.v_means2d_abs is not None:  # (the composite backward ran just before: RasterFn)
                            x.absgrad = st.v_means2d_abs[s:s + 1]

                m2d.register_hook(_deposit)
            self._current_xys = xys
            self._current_radii = [res["radii"][s:s + 1] for s in range(S)]
            self._current_img_wh = img_wh

        assert blended.shape[-1] == sum(ds_expected.values())
        out_dict = {}
        for (name, dim), x in zip(ds_expected.items(), torch.split(blended, list(ds_expected.values()), dim=-1)):
            out_dict[name] = x.reshape(1, H, W, B, 3) if name == "tracks_3d" else x
        out_dict["acc"] = res["acc"][None, ..., None]
        out_dict["deltaT"] = deltaT.unsqueeze(0)
        out_dict["RTs"] = RTs_s
        exposure = renders[:, None]  # [S,1,H,W,D']
        if self.inplace_blend_quirk:
            exposure = torch.cat([exposure[:-1], blended[None]], 0)
        if target_ts is not None:
            out_dict["pred_sharp_img"] = (blended if S == 1 else renders[S // 2][None])[..., 0:3]
        out_dict["exposure_imgs"] = exposure
        return out_dict


@torch.inference_mode()
def render_view(model: SceneModel, t, c2w: torch.Tensor, fov: float, img_wh: tuple[int, int]) -> torch.Tensor:
    """The arithmetic of the viewer callback `Renderer.render_fn` (flow3d/renderer.py:57-89) without the viser /
    nerfview plumbing: K from the vertical fov, w2c = inv(c2w), `render(...)["img"][0]` -> uint8 [H,W,3]."""
    import math

    W, H = img_wh
    focal = 0.5 * H / math.tan(0.5 * fov)
    K = torch.tensor([[focal, 0.0, W / 2.0], [0.0, focal, H / 2.0], [0.0, 0.0, 1.0]], device=c2w.device)
    w2c = torch.linalg.inv(c2w.float())
    img = model.render(t, w2c[None], K[None], img_wh)["img"][0]
    return (img * 255.0).to(torch.uint8)
