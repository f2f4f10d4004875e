"""The Adam parity case shared by tests/test_adam_cpu.py and tests/test_gpu_adam.py: a table of mixed tensors, 50 steps of
seeded fp32 gradients, the fp64 truth and the fp32 yardstick - both `torch.optim.Adam(foreach=False, fused=False)` on the CPU,
one optimizer per tensor, fed the same fp32 gradients."""
import torch

SHAPES = [(1,), (3,), (4,), (5,), (63,), (64,), (65,), (40_000, 20)]
LRS = [1.6e-4, 1e-2, 5e-3, 5e-4, 2e-3, 1e-3, 3e-3, 7e-3]            # distinct per tensor
EPSS = [1e-8, 1e-15, 1e-6, 3e-8, 1e-7, 2e-8, 5e-8, 1e-10]           # distinct per tensor
STEPS = 50
SKIPPED = 6                                # the [65] tensor receives no gradient ...
SKIP_STEPS = {0, 3, 4, 17, 30, 31, 32}     # ... on these steps (step 0 too: its state is then created one step later)


def initial_params():
    g = torch.Generator().manual_seed(20)
    return [torch.randn(s, generator=g) for s in SHAPES]


def gradient(step: int, i: int):
    """fp32 gradient of tensor i at `step` (None: no gradient): a per-tensor mean plus noise, so neither moment averages out."""
    if i == SKIPPED and step in SKIP_STEPS:
        return None
    base = torch.randn(SHAPES[i], generator=torch.Generator().manual_seed(7000 + i))
    noise = torch.randn(SHAPES[i], generator=torch.Generator().manual_seed(100_000 + 64 * step + i))
    return (base + 0.5 * noise) * (0.1 if i % 2 else 3e-3)


def run(make, dtype=torch.float32, device="cpu", on_step=None):
    """make(params) -> (step_fn, state_of(i) -> dict with step / exp_avg / exp_avg_sq, empty before the first gradient).  Returns per tensor
    (param, exp_avg, exp_avg_sq, step) as fp64 CPU tensors / a float."""
    params = [p.to(dtype).to(device).requires_grad_() for p in initial_params()]
    step_fn, state_of = make(params)
    for s in range(STEPS):
        for i, p in enumerate(params):
            g = gradient(s, i)
            p.grad = None if g is None else g.to(dtype).to(device)
        if on_step is not None:
            on_step(s, params, state_of, step_fn)
        else:
            step_fn()
    out = []
    for i, p in enumerate(params):
        st = state_of(i)
        out.append((p.detach().double().cpu(), st["exp_avg"].double().cpu(), st["exp_avg_sq"].double().cpu(), float(st["step"])))
    return out


def torch_adam(params):
    opts = [torch.optim.Adam([p], lr=LRS[i], eps=EPSS[i], foreach=False, fused=False) for i, p in enumerate(params)]

    def step_fn():
        for o in opts:
            o.step()

    return step_fn, lambda i: opts[i].state.get(params[i], {})


def errors(result, truth):
    """Per tensor: max-abs error of (param, exp_avg, exp_avg_sq) against the truth."""
    return [tuple((a - b).abs().max().item() for a, b in zip(r[:3], t[:3])) for r, t in zip(result, truth)]


def table(yard, ours, title):
    lines = [f"# {title}", "",
             f"{STEPS} steps; max-abs error against torch.optim.Adam in fp64 (same fp32 gradients).  Yardstick: torch.optim.Adam "
             "(foreach=False, fused=False) in fp32 on the CPU.  Asserted: ours <= 2 x yardstick, per tensor and quantity.", "",
             "| tensor | lr | eps | param: yardstick | param: ours | exp_avg: yardstick | exp_avg: ours | exp_avg_sq: yardstick | exp_avg_sq: ours |",
             "|---|---:|---:|---:|---:|---:|---:|---:|---:|"]
    for i, (y, o) in enumerate(zip(yard, ours)):
        lines.append(f"| {list(SHAPES[i])} | {LRS[i]:g} | {EPSS[i]:g} | " + " | ".join(f"{y[k]:.3e} | {o[k]:.3e}" for k in range(3)) + " |")
    return "\n".join(lines) + "\n"
