"""Two builds of libd4gs.so give the same bits in every loss and metric that sums in a fixed order (csrc/reduce.h) and in the
rasterizer's forward and backward - and the losses take the same time.

    python scripts/ab_bitwise.py PARENT.so [NEW.so] [--times | --front] [--rounds 2] [--out FILE]

PARENT.so: the parent commit's library (export it with `git archive <parent>` into the git-ignored scripts/ablate/parent/, build it there
with `python -m deblur4dgs_amd.build --force`); NEW.so defaults to this tree's deblur4dgs_amd/libd4gs.so.  D4GS_LIB_PATH is read when
the package loads the library, so every library gets a fresh child process of its own, each under its own `timeout`; the chain stops
at the first child that fails.

Digests (the default): each child runs seeded cases through the public entry points - photometric_loss, masked_l1_loss,
trimmed_l1_loss, compute_gradient_loss, track_losses, motion_regularizers, masked_image_metrics with and without SSIM, the aligned-L1
path of pwcnet, spherical harmonics forward and backward with a view-origin gradient - forward and backward, at two sizes: a smallest
shape of the loss's GPU test and one whose count of block partials exceeds 256 (aligned L1 caps its partials at 128 per pair: that
size), and prints the sha256 of every output and gradient.  The rasterizer's cases (_raster_cases) follow, at 6 000 splats on 200 x 120
and 30 000 on 320 x 200.  The script fails if a digest differs between the libraries.

--front: the digests of the list front end's and the projection backward's cases instead (_front_cases: one per launch rule of
csrc/host.h's FrontPlan and of project_bwd.hip), plain and with each of the three hooks the tests keep set in a child of its own.

--times: the losses at their own benchmarks' sizes (scripts/bench_photometric.py, bench_metrics.py, bench_trimmed.py, bench_aligned.py's
frame and pair count for the aligned L1 alone, bench_sh.py's first configuration, the regularizers at the size of
profiles/motion_regs_step_times.json), forward + backward captured once into a HIP graph, device events around windows of replays;
parent and new alternate, --rounds children each, and the new library's median is held against the spread of the parent's own runs.
"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_SECONDS = 420


# ---- the cases: name -> (builder(size) -> callable returning the outputs and gradients).  size: "small" | "large" | "bench" ----

def _cases():
    import torch

    sys.path.insert(0, ROOT)
    from deblur4dgs_amd import losses as Ls
    from deblur4dgs_amd import metrics as M
    from deblur4dgs_amd import pwcnet as P
    from deblur4dgs_amd.sh import SHFn

    dev = "cuda:0"

    def rnd(seed):
        g = torch.Generator().manual_seed(seed)
        return (lambda *s: torch.rand(*s, generator=g)), (lambda *s: torch.randn(*s, generator=g))

    def fwd_bwd(fn, leaves):
        xs = [x.clone().requires_grad_() for x in leaves]
        out = fn(*xs)
        outs = list(out) if isinstance(out, (tuple, list)) else [out]
        total = sum((1.0 + 0.5 * i) * o.sum() for i, o in enumerate(outs))
        total.backward()
        return [o.detach() for o in outs] + [x.grad for x in xs]

    def photometric(size):
        B, H, W = {"small": (3, 16, 11), "large": (1, 288, 512), "bench": (1, 288, 512)}[size]
        u, n = rnd(1)
        gt = u(B, H, W, 3)
        pred = (gt + 0.1 * n(B, H, W, 3)).clamp(0, 1).to(dev)
        mask = (u(B, H, W, 1) > 0.3).float().to(dev)
        gt = gt.to(dev)
        return lambda: fwd_bwd(lambda x: Ls.photometric_loss(x, gt, mask, return_terms=True), [pred])

    def depth_inputs(size, seed):
        shape = {"small": (1, 3, 5, 1), "large": (1, 640, 1000, 1), "bench": (1, 288, 512, 1)}[size]
        u, n = rnd(seed)
        gt = 1.0 / (2.0 + 3.0 * u(*shape))
        pred = (gt * (1.0 + 0.1 * n(*shape))).to(dev)
        mask = (u(*shape) < 0.8).float().to(dev)
        return pred, gt.to(dev), mask

    def masked_l1(size):
        pred, gt, mask = depth_inputs(size, 2)
        return lambda: fwd_bwd(lambda x: Ls.masked_l1_loss(x, gt, mask, quantile=0.98), [pred])

    def trimmed_l1(size):
        pred, gt, _ = depth_inputs(size, 3)
        return lambda: fwd_bwd(lambda x: Ls.trimmed_l1_loss(x, gt, 0.9), [pred])

    def gradient_loss(size):
        pred, gt, mask = depth_inputs(size, 4)
        valid = mask > 0.5
        if size == "small":
            valid = torch.ones_like(valid)
        return lambda: fwd_bwd(lambda x: Ls.compute_gradient_loss(x, gt, valid, quantile=0.95), [pred])

    def tracks(size):
        # distinct query pixels in raster order: every gradient address gets one add onto zero, so the scatter is bitwise too
        N, Pq, H, W = {"small": (1, 1, 12, 16), "large": (4, 140000, 400, 400), "bench": (7, 4096, 288, 512)}[size]
        u, n = rnd(5)
        g = torch.Generator().manual_seed(55)
        idx = torch.sort(torch.randperm(H * W, generator=g)[:Pq]).values
        q = torch.stack([idx % W, idx // W], -1).float() + 0.5
        K = torch.eye(3).repeat(N, 1, 1)
        K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2] = 300.0, 300.0, W / 2, H / 2
        z = 1.0 + 4.0 * u(1, H, W, N)
        t3 = torch.stack([(u(1, H, W, N) - 0.5) * z, (u(1, H, W, N) - 0.5) * z, z], -1).to(dev)
        kw = dict(query_tracks_2d=q.to(dev), target_Ks=K.to(dev), target_tracks_2d=(torch.tensor([W, H]) * u(N, Pq, 2)).to(dev),
                  target_visibles=(u(N, Pq) < 0.7).to(dev), track_weights=(0.1 + u(N * Pq)).to(dev),
                  target_track_depths=(1.0 + 4.0 * u(N, Pq)).to(dev))
        return lambda: fwd_bwd(lambda x: Ls.track_losses(x, quantile=0.98, **kw), [t3])

    def motion(size):
        G, K, T, B = {"small": (1, 1, 3, 1), "large": (70000, 32, 2100, 2), "bench": (40000, 20, 7, 8)}[size]
        u, n = rnd(6)
        rots = torch.eye(3)[:2].reshape(6).expand(K, T, 6) + 0.1 * n(K, T, 6)
        leaves = [n(G, 3), n(G, K), rots, 0.1 * n(K, T, 3), 0.3 * n(G, 3)]  # means, motion_coefs, rots, transls, scales
        ts = (u(B) * (T - 1)).to(dev)
        w2c = torch.eye(4).repeat(B, 1, 1)
        w2c[:, :3, :3] += 0.05 * n(B, 3, 3)
        w2c[:, :3, 3] = n(B, 3) + torch.tensor([0.0, 0.0, 6.0])
        w2c = w2c.to(dev)
        leaves = [x.to(dev) for x in leaves]
        return lambda: fwd_bwd(lambda m, c, r, t, s: Ls.motion_regularizers(m, c, r, t, s, ts, w2c), leaves)

    def metrics(size, ssim):
        shapes = {"small": [(1, 1, 11, 11)], "large": [(3, 1, 288, 512)], "bench": [(3, 1, 288, 512), (3, 1, 720, 1280)]}[size]
        data = []
        for Mm, B, H, W in shapes:
            u, n = rnd(7 + H)
            target = u(B, H, W, 3)
            pred = (target + 0.1 * n(B, H, W, 3)).clamp(0, 1).to(dev)
            masks = (u(Mm, B, H, W) < 0.9).float().to(dev)
            data.append((pred, target.to(dev), masks))

        def run():
            with torch.no_grad():
                return [o for pred, target, masks in data for o in M.masked_image_metrics(pred, target, masks, ssim=ssim) if torch.is_tensor(o)]
        return run

    def aligned(size):
        Pn, H, W = {"small": (2, 8, 12), "large": (3, 288, 512), "bench": (20, 288, 512)}[size]
        u, n = rnd(8)
        pred, target, flow = u(Pn, 3, H, W).to(dev), u(Pn, 3, H, W).to(dev), (3.0 * n(Pn, 2, H, W)).to(dev)
        mask = (0.2 + 0.8 * u(Pn, 1, H, W)).to(dev)
        if size == "bench":  # as the training step calls it: the gradient goes to pred
            return lambda: fwd_bwd(lambda p: P.aligned_l1(p, flow, target, mask), [pred])
        # the scatter onto pred's gradient uses float atomics and is not bitwise (csrc/warp.hip): digest the losses and the target's gradient
        return lambda: fwd_bwd(lambda t: P.aligned_l1(pred, flow, t, mask), [target])

    def sh(size):
        d, K, N = {"small": (2, 9, 1), "large": (3, 16, 70001), "bench": (3, 16, 1 << 20)}[size]
        u, n = rnd(9)
        p, o, c = (4 * n(N, 3)).to(dev), torch.tensor([0.1, -0.2, -3.0]).to(dev), (0.3 * n(N, K, 3)).to(dev)
        return lambda: fwd_bwd(lambda pp, oo, cc: SHFn.apply(d, pp, oo, cc, None, True), [p, o, c])

    return {"photometric_loss": photometric, "masked_l1_loss": masked_l1, "trimmed_l1_loss": trimmed_l1, "compute_gradient_loss": gradient_loss,
            "track_losses": tracks, "motion_regularizers": motion, "masked_image_metrics ssim": lambda s: metrics(s, True),
            "masked_image_metrics psnr only": lambda s: metrics(s, False), "aligned_l1": aligned, "sh fwd+bwd with origin": sh}


def _raster_cases():
    """rasterization() forward + backward - every output and every leaf gradient - over the composite kernels' instantiations: channel
    counts on both of the forward's loops and on the matrix-pipe kernels, depth modes, absgrad, antialiased, depth segments, lazy lists,
    exact tiles; and one one-call frame of S = 4 sub-samples, whose backward folds the blend's adjoint into the composite's prologue.
    The composite backward sums in a fixed order (tests/test_gpu_rasterization.py: test_backward_is_deterministic)."""
    import torch

    sys.path.insert(0, ROOT)
    from deblur4dgs_amd.exposure import render_exposure
    from deblur4dgs_amd.rasterization import rasterization
    from deblur4dgs_amd.synth import make_scene
    from tests.util import static_inputs

    dev = "cuda:0"
    shapes = {"small": dict(N=6000, W=200, H=120, seed=77, scale_mul=3.0), "large": dict(N=30000, W=320, H=200, seed=55, scale_mul=2.5)}

    def raster(mode, D, bg=False, env=None, **kw):
        def make(size):
            sh = shapes[size]
            inp = {k: v.to(dev) for k, v in static_inputs(**sh, D=max(D, 1)).items()}
            W, H = sh["W"], sh["H"]
            g = torch.Generator().manual_seed(11)
            nch = D + (mode != "RGB")
            wc, wa = torch.randn(1, H, W, nch, generator=g).to(dev), torch.randn(1, H, W, 1, generator=g).to(dev)
            back = torch.linspace(0.2, 0.9, D)[None].to(dev) if bg else None

            def run():
                leaves = [inp[k].clone().requires_grad_() for k in ("means", "quats", "scales", "opac", "colors", "V")]
                old = {k: os.environ.get(k) for k in (env or {})}
                os.environ.update(env or {})  # (the library reads these per call)
                try:
                    rc, ra, info = rasterization(*leaves[:5], leaves[5][None], inp["K"][None], W, H, backgrounds=back, render_mode=mode, **kw)
                    ((rc * wc).sum() + (ra * wa).sum()).backward()
                    torch.cuda.synchronize()
                finally:
                    for k, v in old.items():
                        os.environ.pop(k) if v is None else os.environ.__setitem__(k, v)
                grads = [x.grad for x in leaves if x.grad is not None]  # (depth only: the colours are not composited)
                extra = [info["means2d"].absgrad] if kw.get("absgrad") else []
                return [rc.detach(), ra.detach(), info["last_ids"]] + grads + extra
            return run
        return make

    def frame(size):
        N, G, K_, S, W, H = {"small": (600, 400, 3, 4, 64, 48), "large": (5000, 3000, 4, 4, 160, 96)}[size]
        sc = make_scene(N, G, K_, S, W, H, seed=31)
        names = ("means", "quats", "scales", "opacities", "colors", "motion_coefs", "rots", "transls", "times", "RTs", "viewmat")
        K = sc["K"].to(dev)
        g = torch.Generator().manual_seed(7)
        wb, wa = torch.randn(H, W, 4, generator=g).to(dev), torch.randn(H, W, generator=g).to(dev)

        def run():
            L = {k: sc[k].to(dev).clone().requires_grad_() for k in names}
            r = render_exposure(*(L[k] for k in names[:5]), 3, *(L[k] for k in names[5:]), K, W, H, background=torch.linspace(0.2, 0.9, 3).to(dev),
                                return_depth=True, blend=True, fused=True)
            assert r["state"].frame_io
            ((r["blended"] * wb).sum() + (r["acc"] * wa).sum()).backward()  # gradients on the blended frame only: the folded adjoint
            torch.cuda.synchronize()
            return [r["blended"].detach(), r["acc"].detach(), r["renders"].detach(), r["alphas"].detach()] + [L[k].grad for k in names]
        return run

    seg = {"D4GS_SEG": "1"}
    return {"raster RGB 1": raster("RGB", 1), "raster RGB+ED 3 bg": raster("RGB+ED", 3, bg=True), "raster RGB 4": raster("RGB", 4),
            "raster RGB+D 5": raster("RGB+D", 5), "raster RGB 8": raster("RGB", 8), "raster RGB+ED 16": raster("RGB+ED", 16),
            "raster ED": raster("ED", 0), "raster RGB+ED 3 absgrad": raster("RGB+ED", 3, absgrad=True),
            "raster RGB+ED 3 antialiased": raster("RGB+ED", 3, rasterize_mode="antialiased"),
            "raster RGB+ED 3 segments": raster("RGB+ED", 3, env=seg), "raster RGB+ED 16 segments": raster("RGB+ED", 16, env=seg),
            "raster RGB+ED 3 lazy_sort": raster("RGB+ED", 3, lazy_sort=True), "raster RGB+ED 3 exact_tiles": raster("RGB+ED", 3, exact_tiles=True),
            "frame S=4 one call": frame}


# the (N, lazy lists, instances per lane) rows of the list front end at S = 64 on 64 x 64: tests/test_gpu_front_plan.py derives them
HOOKS = ("D4GS_COUNT_IN_PROJECT", "D4GS_NO_FUSED_SCAN", "D4GS_SORT_NO_MERGE_LONG")  # --front: one more child per library with each set


def _front_cases():
    """The list front end and the projection backward, one case per launch rule of csrc/host.h's FrontPlan and of project_bwd.hip: every
    instances-per-lane arm of k_count_tiles / k_emit; k_project_fwd<XT, TAB, AA> in all eight combinations (exact tiles, K = 12 against
    K = 6 for the bases table, antialiased) on a dynamic scene of S = 8; one sub-sample group (>= 1 536 blocks) against several; the
    three tails of launch_project_bwd - n_shared <= 160 (S = 1, K = 6), the one-block k_finish (S = 8, K = 6, T = 10), the two launches
    (S = 8, K = 20: n_shared 1 548; K = 6, T = 160: 8 640 leaf elements); the sub-group mappings S = 1, 2, 4 and the poses adjoint; the
    one-call frame with the blend's adjoint folded (D = 3) and launched (D = 16); a backward without D4gsProjOut.blend_bases; a scene of
    mostly short lists with some of 513 ... 2 048 keys (tests/ladder.py "mid": the merge_long regime)."""
    import torch

    sys.path.insert(0, ROOT)
    from deblur4dgs_amd import engine
    from deblur4dgs_amd.exposure import render_exposure
    from deblur4dgs_amd.synth import make_scene
    from tests import ladder, test_gpu_front_plan as fp
    from tests.test_gpu_list_edges import _render as ladder_render

    dev = "cuda:0"
    names = ("means", "quats", "scales", "opacities", "colors", "motion_coefs", "rots", "transls", "times", "RTs", "viewmat")
    small_only = lambda run: (lambda size: run if size == "small" else (lambda: []))

    def arm(N, lazy):
        def run():
            leaves, w2c, K = fp._scene(N)
            r, offs, ids = fp._render(leaves, w2c, K, fp.S, lazy)
            return [r["renders"], r["alphas"], r["means2d"], r["radii"], offs] + ([] if lazy else [ids[:int(offs[-1])]])
        return small_only(run)

    def dynamic(N, G, K_, S, T=24, D=3, W=96, H=64, fused=False, drop_table=False, **kw):
        def run():
            sc = make_scene(N, G, K_, S, W, H, seed=41, T=T, D=D, cam_jitter=0.01)
            L = {k: sc[k].to(dev).clone().requires_grad_() for k in names}
            g = torch.Generator().manual_seed(5)
            wb, wa = torch.randn(H, W, D + 1, generator=g).to(dev), torch.randn(H, W, generator=g).to(dev)
            r = render_exposure(*(L[k] for k in names[:5]), min(D, 3), *(L[k] for k in names[5:]), sc["K"].to(dev), W, H, return_depth=True,
                                blend=True, fused=fused, lazy_sort=False, **kw)
            assert bool(r["state"].frame_io) == fused
            if drop_table:
                r["state"].proj_out["blend_bases"] = None
            ((r["blended"] * wb).sum() + (r["acc"] * wa).sum()).backward()
            torch.cuda.synchronize()
            return [r["blended"].detach(), r["acc"].detach(), r["renders"].detach(), r["means2d"].detach(), r["radii"]] + [L[k].grad for k in names]
        return small_only(run)

    def one_group():
        leaves, w2c, K = fp._scene(400000)  # 1 563 blocks of 256: one sub-sample group
        r, offs, ids = fp._render(leaves, w2c, K, 2, False)
        return [r["renders"], r["means2d"], r["radii"], offs, ids[:int(offs[-1])]]

    def poses():
        sc = make_scene(3000, 2000, 6, 4, 64, 48, seed=43)
        L = [sc[k].to(dev).clone().requires_grad_() for k in ("means", "quats", "motion_coefs", "rots", "transls")]
        m, q, _ = engine.poses(*L, sc["times"].to(dev))
        g = torch.Generator().manual_seed(6)
        ((m * torch.randn(m.shape, generator=g).to(dev)).sum() + (q * torch.randn(q.shape, generator=g).to(dev)).sum()).backward()
        torch.cuda.synchronize()
        return [m.detach(), q.detach()] + [x.grad for x in L]

    def mid_lists():
        sc = ladder.build("mid")
        engine._SIZE_GUESS.clear()
        rc, ra, info, _ = ladder_render(sc, "RGB")
        torch.cuda.synchronize()
        return [rc, ra, info["flatten_ids"], info["isect_offsets"]]

    cases = {f"front N={N}{' lazy' if lazy else ''} (per lane: {pt})": arm(N, lazy) for N, lazy, pt in fp.ROWS}
    for xt in (False, True):
        for K_ in (6, 12):
            for aa in (False, True):
                cases[f"project XT={int(xt)} TAB={int(K_ >= 10)} AA={int(aa)} S=8"] = dynamic(2500, 1500, K_, 8, exact_tiles=xt, antialiased=aa)
    cases["project one sub-sample group"] = small_only(one_group)
    cases["project_bwd tail n_shared<=160 (S=1 K=6)"] = dynamic(2500, 1500, 6, 1)
    cases["project_bwd tail one-block k_finish (S=8 K=6 T=10)"] = dynamic(2500, 1500, 6, 8, T=10)
    cases["project_bwd tail two launches (S=8 K=20)"] = dynamic(2500, 1500, 20, 8)
    cases["project_bwd tail two launches (K=6 T=160)"] = dynamic(2500, 1500, 6, 8, T=160)
    cases["project_bwd sub-groups S=2"] = dynamic(2500, 1500, 6, 2)
    cases["project_bwd sub-groups S=4"] = dynamic(2500, 1500, 6, 4)
    cases["poses fwd + adjoint"] = small_only(poses)
    cases["frame one call, blend adjoint folded (D=3)"] = dynamic(2500, 1500, 6, 4, fused=True)
    cases["frame one call, k_blend_bwd (D=16)"] = dynamic(2500, 1500, 6, 4, D=16, fused=True)
    cases["backward without blend_bases"] = dynamic(2500, 1500, 6, 4, drop_table=True)
    cases["lists mid (merge_long)"] = small_only(mid_lists)
    return cases


def child(times, iters, windows, front=False):
    import torch

    assert torch.cuda.is_available(), "ab_bitwise.py runs on the GPU"
    cases = _front_cases() if front else _cases() if times else {**_cases(), **_raster_cases()}  # (the composites are timed by bench.py, not here)
    for name, make in cases.items():
        if not times:
            for size in ("small", "large"):
                outs = make(size)()
                torch.cuda.synchronize()
                for i, o in enumerate(outs):
                    h = hashlib.sha256(o.detach().contiguous().cpu().numpy().tobytes()).hexdigest()
                    print(f"DIGEST {name} | {size} | {i} {tuple(o.shape)} | {h}", flush=True)
            continue
        fn = make("bench")
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()  # replayed from a graph: the host's own time per call is several times the kernels' and noisier
        with torch.cuda.graph(graph):
            keep = fn()  # noqa: F841  (the graph's outputs stay alive)
        for _ in range(20):
            graph.replay()
        torch.cuda.synchronize()
        us = []
        for _ in range(windows):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                graph.replay()
            e1.record()
            torch.cuda.synchronize()
            us.append(1e3 * e0.elapsed_time(e1) / iters)
        print("TIME " + json.dumps({"case": name, "median_us": statistics.median(us), "min_us": min(us), "max_us": max(us)}), flush=True)


def run_child(lib, extra, env_extra=None):
    env = dict(os.environ, D4GS_LIB_PATH=os.path.abspath(lib), **(env_extra or {}))
    cmd = ["timeout", "-k", "10", str(CHILD_SECONDS), sys.executable, os.path.abspath(__file__), "--child", *extra]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, cwd=ROOT)
    if r.returncode != 0:
        sys.stdout.write(r.stdout[-4000:] + r.stderr[-4000:])
        raise SystemExit(f"the child of {lib} ended with status {r.returncode}: stopping here")
    return r.stdout.splitlines()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent", nargs="?")
    ap.add_argument("new", nargs="?", default=os.path.join(ROOT, "deblur4dgs_amd", "libd4gs.so"))
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--times", action="store_true")
    ap.add_argument("--front", action="store_true")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--iters", type=int, default=500)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.times, a.iters, a.windows, a.front)
    if not a.parent:
        ap.error("the parent commit's library is required")
    sha = lambda p: hashlib.sha256(open(p, "rb").read()).hexdigest()
    lines = [f"parent {sha(a.parent)}  {os.path.relpath(a.parent, ROOT)}", f"new    {sha(a.new)}  {os.path.relpath(a.new, ROOT)}"]
    ok = True
    if not a.times:
        dig = {"parent": {}, "new": {}}
        # --front: the front end's cases, once plain and once per kept hook (read once per process: a child of its own each)
        runs = [("", {})] + [(f"[{h}=1] ", {h: "1"}) for h in HOOKS] if a.front else [("", {})]
        for prefix, hook in runs:
            for tag, lib in (("parent", a.parent), ("new", a.new)):
                out = run_child(lib, ["--front"] if a.front else [], hook)
                dig[tag].update({prefix + k: v for k, v in (ln[7:].rsplit(" | ", 1) for ln in out if ln.startswith("DIGEST "))})
        assert dig["parent"] and dig["parent"].keys() == dig["new"].keys(), "the two children did not run the same cases"
        for k, h in dig["parent"].items():
            same = dig["new"][k] == h
            ok &= same
            lines.append(f"{'equal ' if same else 'DIFFER'} {k} | {h[:16]} {'' if same else dig['new'][k][:16]}")
        lines.append(f"{len(dig['parent'])} digests, {'every one equal' if ok else 'NOT all equal'}")
    else:
        runs = {"parent": [], "new": []}
        for _ in range(a.rounds):
            for tag, lib in (("parent", a.parent), ("new", a.new)):
                out = run_child(lib, ["--times", "--iters", str(a.iters), "--windows", str(a.windows)])
                runs[tag].append({r["case"]: r for r in (json.loads(ln[5:]) for ln in out if ln.startswith("TIME "))})
        lines.append(f"us per forward + backward (graph replay); {a.rounds} processes per library, alternating; each figure the median of {a.windows} windows of {a.iters} graph replays")
        lines.append(f"{'case':34s} {'parent runs':>24s} {'parent spread':>14s} {'new runs':>24s} {'new median':>11s}  verdict")
        for case in runs["parent"][0]:
            p = [r[case]["median_us"] for r in runs["parent"]]
            n = [r[case]["median_us"] for r in runs["new"]]
            spread, med = max(p) - min(p), statistics.median(n)
            inside = min(p) - spread <= med <= max(p) + spread
            ok &= med <= max(p) + spread
            lines.append(f"{case:34s} {' '.join(f'{x:.1f}' for x in p):>24s} {spread:14.2f} {' '.join(f'{x:.1f}' for x in n):>24s} {med:11.1f}  "
                         f"{'inside the parent runs or within their spread' if inside else ('FASTER than the parent by more than its spread' if med < min(p) else 'SLOWER than the parent by more than its spread')}")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "a") as f:
            f.write(text)
    if not ok:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
