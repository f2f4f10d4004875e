"""Multi-tensor Adam: every per-tensor optimizer of a training step in ONE HIP launch (csrc/adam.hip, `d4gs_adam_step`).

The reference trains with one `torch.optim.Adam` per parameter tensor (flow3d/trainer.py:1168-1196) so that the control steps
can re-key each one on its own.  `AdamGroup` keeps that shape - `group.adam(param, lr)` returns a real `torch.optim.Adam`
subclass with one param group and the usual `step` / `exp_avg` / `exp_avg_sq` state, so `control.dup_in_optim` & co.,
`LambdaLR`, `state_dict()` / `load_state_dict()` and checkpoints written by `torch.optim.Adam` keep working - but
`group.step()` updates all of them with one kernel that reads a table in DEVICE memory:

* the table (one `D4gsAdamRec` per tensor) is rebuilt when a parameter or state tensor changed identity (control step,
  `load_state_dict`) and re-uploaded - one asynchronous copy from pinned memory, no host sync - when only a gradient tensor or a
  hyper-parameter (an lr a scheduler moved) changed;
* `group.step()` may be captured in a HIP graph (`torch.cuda.graph`) after one eager call created the state: the launch reads
  lr and the step count from device memory, so replays stay valid; call `group.sync()` between replays to push an lr change.
  Gradient tensors that are born during the capture reach the table through a captured kernel whose arguments carry the
  pointers (`d4gs_adam_set_grads`) - a captured copy from host memory would be read again at every replay;
* no CPU fallback: CPU parameters raise.  `adam_step_cpu` is the separate, test-facing door to the CPU twin
  (`d4gs_adam_step_cpu`, the same per-element function compiled for the host).
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib as L

_REC = C.sizeof(L.AdamRec)


def _blocks(n: int) -> int:
    return max(1, -(-n // L.ADAM_CHUNK))  # d4gs_adam_blocks


def _param(h):
    if len(h.param_groups) != 1 or len(h.param_groups[0]["params"]) != 1:
        raise ValueError("an AdamGroup handle holds exactly one parameter tensor in one param group")
    return h.param_groups[0], h.param_groups[0]["params"][0]


def _check_tensor(t, p, what):
    if t.dtype != torch.float32 or t.device != p.device or t.numel() != p.numel() or not t.is_contiguous() or t.is_sparse:
        raise ValueError(f"HIP Adam needs a dense contiguous float32 {what} of the parameter's size on its device; got "
                         f"{t.dtype}, {tuple(t.shape)}, {t.device}")


def _state(h, p, create: bool):
    """The handle's state dict for `p` (None if there is none yet and `create` is false), with `step` as a float32 scalar
    tensor on the parameter's device - where torch's own capturable / fused Adam keeps it."""
    st = h.state.get(p)
    if not st:
        if not create:
            return None
        st = h.state[p]
        st["step"] = torch.zeros((), dtype=torch.float32, device=p.device)
        st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
    step = st["step"]
    if not (torch.is_tensor(step) and step.dtype == torch.float32 and step.device == p.device and step.numel() == 1):
        st["step"] = torch.as_tensor(step, dtype=torch.float32).reshape(()).to(p.device)  # (a checkpoint of a CPU-`step` Adam)
    _check_tensor(st["exp_avg"], p, "exp_avg")
    _check_tensor(st["exp_avg_sq"], p, "exp_avg_sq")
    return st


def _record(h, create: bool):
    """(param, grad | None, state, (lr, beta1, beta2, eps)) of a handle, or None while it has neither state nor gradient
    (torch creates the state at the first step that sees a gradient, and skips `grad is None` ever after)."""
    grp, p = _param(h)
    if grp["weight_decay"] != 0 or grp["amsgrad"] or grp["maximize"]:
        raise ValueError("HIP Adam implements torch.optim.Adam's defaults only: no weight decay, no amsgrad, no maximize")
    if p.dtype != torch.float32 or not p.is_contiguous():
        raise ValueError("HIP Adam needs contiguous float32 parameters")
    g = p.grad
    if g is not None:
        _check_tensor(g, p, "gradient")
    st = _state(h, p, create and g is not None)
    if st is None:
        return None
    b1, b2 = grp["betas"]
    return p, g, st, (float(grp["lr"]), float(b1), float(b2), float(grp["eps"]))


def _fill(rec, p, g, st, hyper):
    rec.param, rec.grad = p.data_ptr(), (None if g is None else g.data_ptr())
    rec.exp_avg, rec.exp_avg_sq, rec.step = st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), st["step"].data_ptr()
    rec.n = p.numel()
    rec.lr, rec.beta1, rec.beta2, rec.eps = hyper


class HipAdam(torch.optim.Adam):
    """The per-tensor handle `AdamGroup.adam` returns: torch.optim.Adam's param group and state layout, stepped by the
    group's HIP kernel.  `step()` updates this tensor alone; `group.step()` all of the group in one launch."""

    def __init__(self, group: "AdamGroup", param: torch.Tensor, lr: float, betas=(0.9, 0.999), eps: float = 1e-8):
        if not torch.is_tensor(param):
            raise TypeError("AdamGroup.adam takes one parameter tensor")
        super().__init__([param], lr=lr, betas=betas, eps=eps, foreach=False, fused=False)
        self._group = group

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._group._launch(only=self)
        return loss

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)  # (new moment tensors: the group rebuilds its table at the next step)
        for p, st in self.state.items():
            if "step" in st:  # torch hands a non-capturable `step` over as it is - the very tensor of the source, on its device
                st["step"] = torch.as_tensor(st["step"], dtype=torch.float32).reshape(()).to(p.device, copy=True)


class AdamGroup:
    """Owner of the device table.  `generation` counts the rebuilds: a graph that captured `step()` is stale once it moved."""

    def __init__(self):
        self.handles: list[HipAdam] = []
        self.generation = 0
        self._structure = None  # identity of what the table's layout hangs on: parameters, moments, step tensors
        self._grads = None      # gradient pointers in the host's view of the table
        self._hyper = None
        self._stale = True      # the device copy differs from the host's view (until the next upload)
        self._slots = []        # pinned staging copies of the table: [tensor, event of the copy that last read it]

    def adam(self, param: torch.Tensor, lr: float, betas=(0.9, 0.999), eps: float = 1e-8) -> HipAdam:
        h = HipAdam(self, param, lr, betas, eps)
        self.handles.append(h)
        return h

    def zero_grad(self, set_to_none: bool = True):
        for h in self.handles:
            h.zero_grad(set_to_none=set_to_none)

    # -----------------------------------------------------------------------------------------------------------------
    def sync(self):
        """Bring the device table up to date with the handles (no launch of the update itself): what `step()` does first,
        and what a caller replaying a captured `step()` does between replays to push a changed lr."""
        capturing = torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()
        items = []
        for h in self.handles:
            L.need_gpu(_param(h)[1], "deblur4dgs_amd.optim", " (no CPU fallback)")
            rec = _record(h, create=not capturing)
            if rec is None:
                if capturing and _param(h)[1].grad is not None:
                    raise RuntimeError("AdamGroup.step() inside a graph capture needs one eager step() first (it creates the state)")
                continue
            items.append((h, *rec))
        structure = tuple((id(h), p.data_ptr(), p.numel(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(),
                           st["step"].data_ptr()) for h, p, g, st, hy in items)
        grads = tuple(0 if g is None else g.data_ptr() for h, p, g, st, hy in items)
        hyper = tuple(hy for h, p, g, st, hy in items)
        if structure != self._structure:
            if capturing:
                raise RuntimeError("AdamGroup: a parameter or state tensor changed since the last eager step(); the table cannot be "
                                   "rebuilt inside a graph capture - call sync() or step() eagerly first")
            self._rebuild(items, structure)
        elif capturing:
            if hyper != self._hyper:
                raise RuntimeError("AdamGroup: an lr changed since the last eager step(); call sync() before the capture")
            if items and (grads != self._grads or self._stale):  # gradients born inside this capture: a captured kernel carries their pointers
                ptrs = (C.c_void_p * len(items))(*[g or None for g in grads])
                L.check(L.lib().d4gs_adam_set_grads(self._table.data_ptr(), len(items), ptrs, L.stream_of(self._table)), "d4gs_adam_set_grads")
                self._stale = True  # on the device the pointers arrive with the first replay; an eager sync() uploads before that
        elif grads == self._grads and hyper == self._hyper and not self._stale:
            return
        self._grads, self._hyper = grads, hyper
        self._keep = [(p, g, st["exp_avg"], st["exp_avg_sq"], st["step"]) for h, p, g, st, hy in items]  # what the table points at
        if not capturing:
            self._upload(items)

    def device_table(self):
        """The table in device memory after `sync()`: a uint8 tensor holding one `D4gsAdamRec` per handle that has state, in the
        handles' order (None while no handle has any).  For a kernel that writes a field of it on the stream - a schedule that moves
        `lr` between graph replays (`scene_init.track_fit_schedule`).  The next upload replaces what such a kernel wrote by the
        handles' own values; uploads happen when a gradient tensor or a host-side hyper-parameter changed."""
        self.sync()
        return getattr(self, "_table", None)

    def _rebuild(self, items, structure):
        self._structure, self._index = structure, {id(it[0]): i for i, it in enumerate(items)}
        self.generation += 1
        self._stale = True
        if not items:
            self._table = None
            return
        dev = items[0][1].device
        if any(it[1].device != dev for it in items):
            raise ValueError("an AdamGroup serves the tensors of one device")
        self._device = dev
        self._counts = [_blocks(it[1].numel()) for it in items]
        prefix = [0]
        for c in self._counts:
            prefix.append(prefix[-1] + c)
        self._prefix_host = prefix
        single = [x for c in self._counts for x in (0, c)]  # a [0, blocks] pair per record: the prefix table of a one-record launch
        maps = torch.tensor(prefix + single, dtype=torch.int32).to(dev)
        self._prefix, self._single = maps[:len(prefix)], maps[len(prefix):]
        rec_of_block = torch.tensor([r for r, c in enumerate(self._counts) for _ in range(c)], dtype=torch.int64).to(dev)
        # every workgroup's own copy of its record's step count (why: include/d4gs.h)
        self._block_steps = torch.stack([it[3]["step"].reshape(()) for it in items])[rec_of_block].contiguous()
        self._table = torch.empty(len(items) * _REC, dtype=torch.uint8, device=dev)
        self._slots = []

    def _upload(self, items):
        if not items:
            return
        nbytes = len(items) * _REC
        slot = next((s for s in self._slots if s[1].query()), None)  # a staging copy no pending transfer still reads
        if slot is None:
            slot = [torch.empty(nbytes, dtype=torch.uint8).pin_memory(), torch.cuda.Event()]
            self._slots.append(slot)
        recs = (L.AdamRec * len(items)).from_address(slot[0].data_ptr())
        for rec, (h, p, g, st, hy) in zip(recs, items):
            _fill(rec, p, g, st, hy)
        with torch.cuda.device(self._device):
            self._table.copy_(slot[0], non_blocking=True)
            slot[1].record()
        self._stale = False

    def _launch(self, only=None):
        self.sync()
        for h in ([only] if only is not None else self.handles):
            h._opt_called = True  # what torch's own step() wrapper tells the lr schedulers
        if self._table is None:
            return
        lib, n = L.lib(), len(self._counts)
        if only is None:
            L.check(lib.d4gs_adam_step(self._table.data_ptr(), n, self._prefix.data_ptr(), self._prefix_host[-1],
                                       self._block_steps.data_ptr(), L.stream_of(self._table)), "d4gs_adam_step")
            return
        i = self._index.get(id(only))
        if i is None:
            if only not in self.handles:
                raise ValueError("this handle does not belong to the group")
            return  # neither state nor gradient yet
        L.check(lib.d4gs_adam_step(self._table.data_ptr() + i * _REC, 1, self._single.data_ptr() + 8 * i, self._counts[i],
                                   self._block_steps.data_ptr() + 4 * self._prefix_host[i], L.stream_of(self._table)), "d4gs_adam_step")

    @torch.no_grad()
    def step(self):
        """Adam on every handle's tensor: one launch."""
        self._launch()


def adam_step_cpu(group: AdamGroup):
    """TEST-FACING: one Adam step of every handle of `group` on CPU tensors through the CPU twin `d4gs_adam_step_cpu` - the
    per-element function of the HIP kernel compiled for the host, so its numerics can be checked without a GPU.  Never a
    fallback: `AdamGroup.step()` refuses CPU tensors, and this function refuses device tensors."""
    items = []
    with torch.no_grad():
        for h in group.handles:
            if _param(h)[1].is_cuda:
                raise RuntimeError("adam_step_cpu takes CPU tensors (the device path is AdamGroup.step)")
            rec = _record(h, create=True)
            if rec is not None:
                items.append(rec)
                h._opt_called = True
        recs = (L.AdamRec * max(len(items), 1))()
        for rec, it in zip(recs, items):
            _fill(rec, *it)
        L.check(L.lib().d4gs_adam_step_cpu(recs, len(items)), "d4gs_adam_step_cpu")
