"""FusedSGDTail: the optimizer tail of the reference's step as one capturable call.

Replaces, per step (reference src/scripts/train.py:411-427)

    clip_grad_norm_(net.parameters(), max_grad_norm)     # one norm over all gradients
    optim.step()                                          # src/utils/optimizer.py: host-side warm-up / poly schedule + torch SGD
    ema.update(net)                                       # src/utils/ema.py: two launches per floating-point state_dict entry

by ``cabinet_sgd_tail_step`` (csrc/opt_tail.hip: three launches).  The step counter ``it``, the EMA counter and the learning-rate
schedule live on the device, so the call can be recorded into a hipGraph (``GraphedTrainStep(..., capture_optimizer=True)``) and
every replay still advances the schedule.  Device parameters use the kernels or raise; host parameters take a composite torch path
with the same semantics (what the CPU test tier checks).

Checkpoints interchange with the reference: the momentum buffers live in the ``state`` of an inner, never-stepped
``torch.optim.SGD`` with the reference's group layout, and ``state_dict`` / ``load_state_dict`` / ``param_groups`` delegate to it;
``it`` and ``ema_updates`` are settable, ``ema`` is the averaged module (``ModelEMA.ema``).
"""

from __future__ import annotations

import ctypes
import math
from copy import deepcopy

import numpy as np
import torch

from . import _lib

CHUNK = 4096
EMA_ONLY = 1

_ENTRY = np.dtype([("param", "<u8"), ("grad", "<u8"), ("buf", "<u8"), ("ema", "<u8"), ("numel", "<i8"), ("group", "<i4"),
                   ("flags", "<i4")])
_CHUNK = np.dtype([("start", "<i8"), ("tensor", "<i4"), ("length", "<i4")])
_HEADER_BYTES = 128  # it, updates, skipped (int64) | nonfinite, apply (int32) | norm, coef, lr[4], d, 1-d (float32)


class _Config(ctypes.Structure):
    _fields_ = [("lr0", ctypes.c_double), ("warmup_start_lr", ctypes.c_double), ("max_iter", ctypes.c_double),
                ("power", ctypes.c_double), ("lr_scale", ctypes.c_double * 4), ("weight_decay", ctypes.c_double * 4),
                ("momentum", ctypes.c_double), ("max_norm", ctypes.c_double), ("ema_decay", ctypes.c_double),
                ("ema_tau", ctypes.c_double), ("warmup_steps", ctypes.c_longlong), ("skip_nonfinite", ctypes.c_int),
                ("reserved", ctypes.c_int)]


def _unwrap(model):
    inner = getattr(model, "module", model)
    return inner if isinstance(inner, torch.nn.Module) else model


def _dense(t):
    """Non-overlapping and dense: the elements fill one span of memory exactly (any permutation of a contiguous layout)."""
    expect = 1
    for size, stride in sorted(((s, st) for s, st in zip(t.shape, t.stride()) if s != 1), key=lambda x: x[1]):
        if stride != expect:
            return False
        expect *= size
    return True


def build_chunks(numels):
    """The chunk list of a table: every tensor cut at multiples of CHUNK; a tensor of <= CHUNK elements is one chunk."""
    rows = [(start, i, min(CHUNK, n - start)) for i, n in enumerate(numels) for start in range(0, n, CHUNK)]
    return np.array(rows, dtype=_CHUNK)


class FusedSGDTail:
    capturable = True

    def __init__(self, net, lr0, momentum=0.9, wd=1e-4, warmup_steps=0, warmup_start_lr=1e-5, max_iter=100000, power=0.9,
                 lr_multiplier=10.0, max_grad_norm=1.0, ema=True, ema_decay=0.9999, ema_tau=2000, skip_nonfinite=True):
        self.net = _unwrap(net)
        self.lr0, self.momentum, self.wd = float(lr0), float(momentum), float(wd)
        self.warmup_steps, self.warmup_start_lr = int(warmup_steps), float(warmup_start_lr)
        self.max_iter, self.power, self.lr_multiplier = float(max_iter), float(power), float(lr_multiplier)
        self.max_grad_norm = float(max_grad_norm or 0.0)
        self.ema_decay, self.ema_tau, self.skip_nonfinite = float(ema_decay), float(ema_tau), bool(skip_nonfinite)
        if not self.max_iter > self.warmup_steps >= 0:
            raise ValueError("FusedSGDTail: needs max_iter > warmup_steps >= 0")
        if not self.ema_tau > 0:
            raise ValueError("FusedSGDTail: needs ema_tau > 0")
        # groups exactly as the reference builds them (optimizer.py:56-102)
        if not hasattr(self.net, "get_params"):
            raise RuntimeError("Model must have .get_params() method returning param groups")
        params = self.net.get_params()
        if len(params) == 2:
            params = (*params, [], [])
        elif len(params) != 4:
            raise ValueError(f"Expected 2 or 4 param groups, got {len(params)}")
        groups = []
        for plist, decay, scaled in zip(params, (wd, 0.0, wd, 0.0), (False, False, True, True)):
            if plist:
                g = {"params": list(plist), "weight_decay": decay}
                if scaled:
                    g["lr_scale"] = lr_multiplier
                groups.append(g)
        if not groups:
            raise ValueError("No parameters found in model!")
        # never stepped: it holds the param groups and the momentum buffers in torch's own layout (checkpoint interchange)
        self.optim = torch.optim.SGD(groups, lr=lr0, momentum=momentum, weight_decay=0.0)
        owned = [p for g in self.optim.param_groups for p in g["params"]]
        devices = {p.device for p in owned}
        if len(devices) != 1:
            raise RuntimeError(f"FusedSGDTail: parameters on several devices {sorted(map(str, devices))}")
        self.device = devices.pop()
        if any(p.dtype != torch.float32 for p in owned):
            raise RuntimeError("FusedSGDTail: fp32 parameters only")
        # the averaged copy (ModelEMA.ema): eval mode, no gradients
        if ema is True:
            self.ema = deepcopy(self.net).eval()
        elif ema is None or ema is False:
            self.ema = None
        else:
            self.ema = _unwrap(ema).eval()
        if self.ema is not None:
            for p in self.ema.parameters():
                p.requires_grad_(False)
        # entries: every floating-point state_dict entry, in state_dict order; those the optimizer owns carry group and buffer
        group_of = {id(p): gi for gi, g in enumerate(self.optim.param_groups) for p in g["params"]}
        live = dict(self.net.state_dict(keep_vars=True))
        avg = dict(self.ema.state_dict(keep_vars=True)) if self.ema is not None else {}
        self._names, self._live, self._avg, self._group = [], [], [], []
        seen = set()
        for name, t in live.items():
            if not t.dtype.is_floating_point:
                continue  # integer buffers (num_batches_tracked) are left alone, as ema.py:61-65 does
            gi = group_of.get(id(t))
            if gi is None and self.ema is None:
                continue
            if t.dtype != torch.float32 or t.device != self.device:
                raise RuntimeError(f"FusedSGDTail: state_dict entry {name} is {t.dtype} on {t.device}; fp32 on {self.device} only")
            seen.add(id(t))
            self._names.append(name)
            self._live.append(t)
            self._avg.append(avg.get(name))
            self._group.append(-1 if gi is None else gi)
        missing = [p for p in owned if id(p) not in seen]
        if missing:
            raise RuntimeError(f"FusedSGDTail: {len(missing)} parameters of get_params() are not in the model's state_dict")
        n = len(self._live)
        for p in owned:
            if self.momentum != 0:
                self.optim.state[p]["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        self._chunks_host = build_chunks([t.numel() for t in self._live])
        # device state: header + valid[n] + first[n] (include/cabinet_hip.h), zeroed; the CPU path keeps the same block
        self._on_device = self.device.type == "cuda"
        if self._on_device:
            self._lib = _lib.load()  # a missing library raises here: there is no torch fallback for device parameters
            state_bytes = int(self._lib.cabinet_sgd_tail_state_bytes(n))
            ws_bytes = int(self._lib.cabinet_sgd_tail_workspace_bytes(len(self._chunks_host)))
            self._ws = torch.empty(ws_bytes, dtype=torch.uint8, device=self.device)
            self._chunks = torch.from_numpy(self._chunks_host.view(np.uint8)).to(self.device)
        else:
            state_bytes = _HEADER_BYTES + 8 * n
        self._state = torch.zeros(state_bytes, dtype=torch.uint8, device=self.device)
        self._counters = self._state[0:24].view(torch.int64)       # it, updates, skipped
        self._flags = self._state[24:32].view(torch.int32)         # nonfinite, apply
        self._scalars = self._state[32:64].view(torch.float32)     # norm, coef, lr[4], d, 1 - d
        self._valid = self._state[_HEADER_BYTES:_HEADER_BYTES + 4 * n].view(torch.int32)
        self.last_grad_norm = self._scalars[0:1]
        self.lr = self._scalars[2:6]
        self.max_grid = 0                 # 0: the kernels' own cap; tests force the grid-stride loop with a small value
        self._uploaded = None             # the address tuple the device table was built from
        self._entries = None              # device table
        self._entries_captured = False    # a hipGraph holds the table's address: never overwrite it
        self._keep = []                   # tables held by graphs
        self._cfg = _Config()

    # ------------------------------------------------------------------ reference-compatible surface
    @property
    def param_groups(self):
        return self.optim.param_groups

    @property
    def defaults(self):
        return self.optim.defaults

    def state_dict(self):
        return self.optim.state_dict()

    def load_state_dict(self, state):
        """Loads a checkpoint's ``optimizer_state`` (the reference's or this class's).  Loaded buffers count as valid; a
        parameter without one gets a zero buffer that the next step overwrites, torch's first-step rule."""
        self.optim.load_state_dict(state)
        valid = torch.zeros(len(self._live), dtype=torch.int32)
        index = {id(t): i for i, t in enumerate(self._live)}
        for g in self.optim.param_groups:
            for p in g["params"]:
                if self.momentum == 0:
                    continue
                loaded = self.optim.state[p].get("momentum_buffer")
                buf = torch.zeros_like(p, memory_format=torch.preserve_format)
                if loaded is not None:
                    buf.copy_(loaded)
                    valid[index[id(p)]] = 1
                self.optim.state[p]["momentum_buffer"] = buf
        self._valid.copy_(valid)
        self._uploaded = None  # re-read the addresses

    def zero_grad(self, set_to_none=True):
        self.optim.zero_grad(set_to_none=set_to_none)

    def _read(self, i):
        return int(self._counters[i])

    @property
    def it(self):
        """Optimizer steps taken (reads the device: a sync, meant for epoch ends)."""
        return self._read(0)

    @it.setter
    def it(self, v):
        self._counters[0] = int(v)

    @property
    def ema_updates(self):
        return self._read(1)

    @ema_updates.setter
    def ema_updates(self, v):
        self._counters[1] = int(v)

    @property
    def skipped(self):
        """Steps skipped because the gradient norm was inf / nan."""
        return self._read(2)

    # ------------------------------------------------------------------ step
    def _config(self):
        c, groups = self._cfg, self.optim.param_groups
        c.lr0, c.warmup_start_lr, c.max_iter, c.power = self.lr0, self.warmup_start_lr, self.max_iter, self.power
        for i in range(4):
            g = groups[i] if i < len(groups) else {}
            c.lr_scale[i] = float(g.get("lr_scale", 1.0))
            c.weight_decay[i] = float(g.get("weight_decay", 0.0))
        c.momentum = float(groups[0]["momentum"])
        c.max_norm, c.ema_decay, c.ema_tau = self.max_grad_norm, self.ema_decay, self.ema_tau
        c.warmup_steps, c.skip_nonfinite = self.warmup_steps, int(self.skip_nonfinite)
        return c

    def _rows(self):
        """(param, grad, buffer, ema) tensors per entry; grad None = EMA-only this step."""
        rows = []
        for t, e, gi in zip(self._live, self._avg, self._group):
            if gi < 0 or t.grad is None:
                rows.append((t, None, None, e))
            else:
                rows.append((t, t.grad, self.optim.state[t].get("momentum_buffer"), e))
        return rows

    def _check_row(self, i, p, g, b, e):
        for what, t in (("grad", g), ("buffer", b), ("ema", e)):
            if t is None:
                continue
            if t.dtype != torch.float32 or t.device != p.device or t.shape != p.shape or t.stride() != p.stride():
                raise RuntimeError(f"FusedSGDTail: {what} of {self._names[i]} is {t.dtype} {tuple(t.shape)} strides "
                                   f"{t.stride()} on {t.device}; the parameter is {tuple(p.shape)} strides {p.stride()}: "
                                   "the four tensors of an entry must be dense fp32 with equal strides")
        if not _dense(p):
            raise RuntimeError(f"FusedSGDTail: {self._names[i]} with shape {tuple(p.shape)} and strides {p.stride()} is "
                               "not dense; the four tensors of an entry must be dense with equal strides")

    def _upload(self, rows, key):
        host = np.zeros(len(rows), dtype=_ENTRY)
        for i, (p, g, b, e) in enumerate(rows):
            self._check_row(i, p, g, b, e)
            host[i] = (p.data_ptr(), g.data_ptr() if g is not None else 0, b.data_ptr() if b is not None else 0,
                       e.data_ptr() if e is not None else 0, p.numel(), max(self._group[i], 0), 0 if g is not None else EMA_ONLY)
        dev = torch.from_numpy(host.view(np.uint8)).to(self.device)
        if self._entries is not None and self._entries_captured:
            self._keep.append(self._entries)  # a graph replays from it
        self._entries, self._entries_captured, self._uploaded = dev, False, key

    def prepare_capture(self):
        """Bring the device table up to date with the current addresses.  Call before recording ``step()`` into a graph
        (``_OptimizerSegment.record`` does): inside a capture an address change raises instead."""
        if self._on_device:
            rows = self._rows()
            key = tuple(0 if t is None else t.data_ptr() for r in rows for t in r)
            if key != self._uploaded:
                self._upload(rows, key)

    @torch.no_grad()
    def step(self):
        if not self._on_device:
            return self._step_composite()
        rows = self._rows()
        key = tuple(0 if t is None else t.data_ptr() for r in rows for t in r)
        capturing = torch.cuda.is_current_stream_capturing()
        if key != self._uploaded:
            if capturing:
                raise RuntimeError("FusedSGDTail.step(): a parameter, gradient, momentum-buffer or EMA address changed and the "
                                   "table cannot be uploaded during stream capture; call prepare_capture() before recording")
            self._upload(rows, key)
        if capturing:
            self._entries_captured = True
        rc = self._lib.cabinet_sgd_tail_step(self._entries.data_ptr(), len(rows), self._chunks.data_ptr(), len(self._chunks_host),
                                             ctypes.addressof(self._config()), self._state.data_ptr(), self._state.numel(),
                                             int(self.max_grid), self._ws.data_ptr(), self._ws.numel(),
                                             torch.cuda.current_stream(self.device).cuda_stream)
        _lib.check(rc, "cabinet_sgd_tail_step")

    def _step_composite(self):
        """Host parameters: the same step in torch ops (same order of fp32 operations per element as the kernels)."""
        c = self._config()
        rows = self._rows()
        sumsq = 0.0
        for i, (p, g, b, e) in enumerate(rows):
            self._check_row(i, p, g, b, e)
            if g is not None:
                sumsq += float(g.double().pow(2).sum())
        norm = math.sqrt(sumsq) if sumsq == sumsq else float("nan")
        nonfinite = not math.isfinite(norm)
        self._scalars[0] = norm
        self._flags[0] = int(nonfinite)
        if nonfinite and self.skip_nonfinite:
            self._flags[1] = 0
            self._counters[2] += 1
            return
        self._flags[1] = 1
        coef = min(1.0, c.max_norm / (norm + 1e-6)) if c.max_norm > 0 else 1.0
        it = int(self._counters[0])
        if it < self.warmup_steps:
            lr = self.warmup_start_lr + it / self.warmup_steps * (self.lr0 - self.warmup_start_lr)
        else:
            k = min(max((it - self.warmup_steps) / (self.max_iter - self.warmup_steps), 0.0), 1.0)
            lr = self.lr0 * (1 - k) ** self.power
        updates = int(self._counters[1]) + 1
        d = self.ema_decay * (1 - math.exp(-updates / self.ema_tau))
        self._scalars[1] = coef
        for gi in range(4):
            self._scalars[2 + gi] = lr * c.lr_scale[gi]
        self._scalars[6], self._scalars[7] = d, 1 - d
        self._counters[0], self._counters[1] = it + 1, updates
        for i, (p, g, b, e) in enumerate(rows):
            if g is not None:
                gi = self._group[i]
                g = g * coef
                if c.weight_decay[gi] != 0:
                    g = g.add(p, alpha=c.weight_decay[gi])
                if b is not None and c.momentum != 0:
                    if int(self._valid[i]):
                        b.mul_(c.momentum).add_(g)
                    else:
                        b.copy_(g)
                        self._valid[i] = 1
                    g = b
                p.add_(g, alpha=-float(self._scalars[2 + gi]))
            if e is not None:
                e.mul_(d).add_(p.detach(), alpha=1 - d)


# ---------------------------------------------------------------------------------------------------------------------------------
_ACCUM_ENTRY = np.dtype([("acc", "<u8"), ("grad", "<u8"), ("numel", "<i8")])
_ACCUM_STATE_BYTES = 64  # micro (int32) | reserved


class GradAccumulator:
    """Gradient accumulation across hipGraph replays as one capturable call (csrc/grad_accum.hip, ``cabinet_grad_accum``).

    ``pairs``: a list of ``(acc, grad)`` tensors.  ``add()`` folds every ``grad`` into its ``acc``: a copy when the device counter
    ``micro`` is 0 (``acc`` is not read: a stale NaN does not survive), one fp32 add otherwise -- bit for bit what autograd's own
    accumulation into ``.grad`` gives in the same order -- and advances ``micro``; ``reset()`` sets it to 0.  Nothing is read on the
    host, so ONE recorded ``add()`` serves every micro-step of every window.  Device tensors use the kernel or raise; host tensors
    take a composite torch path with the same semantics (what the CPU test tier checks).

    A ``grad`` of ``None`` in EVERY pair leaves the gradient side open: a captured backward only shows its static gradient tensors
    once it has been recorded, in the capture that also has to record ``add()``.  Recording reads no table, so ``add()`` may be
    recorded on an open accumulator and ``bind(grads)`` called once, after the capture and before the first replay.  That is the
    one write into a table a graph holds; afterwards, as in ``FusedSGDTail``, a table a graph has recorded is never overwritten
    (an address change outside capture uploads a fresh table; inside capture it raises)."""

    def __init__(self, pairs):
        pairs = [tuple(p) for p in pairs]
        if not pairs:
            raise ValueError("GradAccumulator: no tensors")
        self._acc = [a for a, _ in pairs]
        grads = [g for _, g in pairs]
        opened = [g is None for g in grads]
        if any(opened) and not all(opened):
            raise ValueError("GradAccumulator: either every pair names its gradient or none does (bind() names them later)")
        devices = {a.device for a in self._acc}
        if len(devices) != 1:
            raise RuntimeError(f"GradAccumulator: tensors on several devices {sorted(map(str, devices))}")
        self.device = devices.pop()
        for i, a in enumerate(self._acc):
            if a.dtype != torch.float32 or not _dense(a):
                raise RuntimeError(f"GradAccumulator: acc of pair {i} is {a.dtype} {tuple(a.shape)} strides {a.stride()}; the two "
                                   "tensors of a pair must be dense fp32 with equal strides")
        self._chunks_host = build_chunks([a.numel() for a in self._acc])
        if len(self._chunks_host) == 0:
            raise ValueError("GradAccumulator: every tensor is empty")
        self._on_device = self.device.type == "cuda"
        n = len(self._acc)
        if self._on_device:
            self._lib = _lib.load()  # a missing library raises here: there is no torch fallback for device tensors
            state_bytes = int(self._lib.cabinet_grad_accum_state_bytes())
            self._chunks = torch.from_numpy(self._chunks_host.view(np.uint8)).to(self.device)
            self._entries = torch.zeros(n * _ACCUM_ENTRY.itemsize, dtype=torch.uint8, device=self.device)
        else:
            state_bytes = _ACCUM_STATE_BYTES
        self._state = torch.zeros(state_bytes, dtype=torch.uint8, device=self.device)
        self._micro = self._state[0:4].view(torch.int32)
        self.max_grid = 0                 # 0: the kernel's own cap; tests force the grid-stride loop with a small value
        self._grad = None                 # bound gradient tensors
        self._uploaded = None             # the address tuple the device table was built from
        self._entries_captured = False    # a hipGraph holds the table's address: never overwrite it (but for the one bind())
        self._keep = []                   # tables held by graphs
        if not opened[0]:
            self.bind(grads)

    # ------------------------------------------------------------------ tables
    def _check_pair(self, i, a, g):
        if g.dtype != torch.float32 or g.device != a.device or g.shape != a.shape or g.stride() != a.stride():
            raise RuntimeError(f"GradAccumulator: grad of pair {i} is {g.dtype} {tuple(g.shape)} strides {g.stride()} on "
                               f"{g.device}; acc is {a.dtype} {tuple(a.shape)} strides {a.stride()} on {a.device}: the two "
                               "tensors of a pair must be dense fp32 with equal strides")
        if a.numel() and g.data_ptr() == a.data_ptr():
            raise RuntimeError(f"GradAccumulator: acc and grad of pair {i} are the same memory")

    def _key(self):
        return tuple(t.data_ptr() for pair in zip(self._acc, self._grad) for t in pair)

    def _host_table(self):
        host = np.zeros(len(self._acc), dtype=_ACCUM_ENTRY)
        for i, (a, g) in enumerate(zip(self._acc, self._grad)):
            self._check_pair(i, a, g)
            host[i] = (a.data_ptr(), g.data_ptr(), a.numel())
        return torch.from_numpy(host.view(np.uint8))

    def bind(self, grads):
        """Name the gradient side of an open accumulator (once).  Must not be called during stream capture."""
        if self._grad is not None:
            raise RuntimeError("GradAccumulator.bind(): the gradients are already bound")
        grads = list(grads)
        if len(grads) != len(self._acc):
            raise RuntimeError(f"GradAccumulator.bind(): {len(grads)} gradients for {len(self._acc)} accumulation tensors")
        for i, (a, g) in enumerate(zip(self._acc, grads)):
            self._check_pair(i, a, g)
        self._grad = grads
        if self._on_device:
            self._entries.copy_(self._host_table())  # the table's first content: a recorded add() has not run yet
            self._uploaded = self._key()

    @property
    def pairs(self):
        return list(zip(self._acc, self._grad or [None] * len(self._acc)))

    # ------------------------------------------------------------------ counter
    @property
    def micro(self):
        """Micro-steps folded into ``acc`` in the current window (reads the device: a sync)."""
        return int(self._micro[0])

    @micro.setter
    def micro(self, v):
        self._micro[0] = int(v)

    # ------------------------------------------------------------------ calls
    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    @torch.no_grad()
    def add(self):
        if not self._on_device:
            if self._grad is None:
                raise RuntimeError("GradAccumulator.add(): no gradients bound")
            first = self.micro == 0
            for i, (a, g) in enumerate(zip(self._acc, self._grad)):
                self._check_pair(i, a, g)
                if first:
                    a.copy_(g)
                else:
                    a.add_(g)
            self._micro[0] += 1
            return
        capturing = torch.cuda.is_current_stream_capturing()
        if self._grad is None:
            if not capturing:
                raise RuntimeError("GradAccumulator.add(): no gradients bound; an open accumulator can only be recorded")
        elif self._key() != self._uploaded:
            if capturing:
                raise RuntimeError("GradAccumulator.add(): an accumulation or gradient address changed and the table cannot be "
                                   "uploaded during stream capture")
            if self._entries_captured:
                self._keep.append(self._entries)  # a graph replays from it
                self._entries, self._entries_captured = torch.empty_like(self._entries), False
            self._entries.copy_(self._host_table())
            self._uploaded = self._key()
        if capturing:
            self._entries_captured = True
        rc = self._lib.cabinet_grad_accum(self._entries.data_ptr(), len(self._acc), self._chunks.data_ptr(), len(self._chunks_host),
                                          self._state.data_ptr(), self._state.numel(), int(self.max_grid), self._stream())
        _lib.check(rc, "cabinet_grad_accum")

    @torch.no_grad()
    def reset(self):
        """Start a new window: the next ``add()`` copies."""
        if not self._on_device:
            self._micro[0] = 0
            return
        rc = self._lib.cabinet_grad_accum_reset(self._state.data_ptr(), self._state.numel(), self._stream())
        _lib.check(rc, "cabinet_grad_accum_reset")
