"""Training of the LAENeRF palette network on extracted views: the reference's `train_LAENeRF_step` loop (nerf/utils.py:953-1055,
driven 16 steps per call by nerf/gui.py:1997-2026) on a device-resident edit set, one captured HIP graph per buffer capacity.

Per step: the step's view (`lae_sample_edit_view`: the schedule entry at the device step counter, the depth jitter of
`EditDataset.collate`, rows padded to the capacity with copies of the last jittered row, the live row count K in device memory)
-> `LAENeRF.forward_train_loss(..., m_dev=K)` (MSE + weights_loss + offset_loss + palet_loss as one node; rows >= K excluded)
-> FusedAdam's backward and step (its GradScaler) -> the unscaled loss and the MSE recorded on the device at the step's row.

What makes one graph serve many steps although every view has its own K:
  * the host knows each step's view (the schedule is drawn up front), so a step runs at capacity `capacity_for(K)`: 'bucket'
    rounds K up to 8 steps per octave (at most 12.5 % pad rows, few graphs), 'exact' to the next multiple of 16 (a graph per
    distinct K: the no-padding floor);
  * the sampler writes K into device memory and the loss kernels read it there, so a graph captured at a capacity serves every
    view that fits it.  Pad rows are copies of a real row: they touch only hash-table lines the view touches, so FusedAdam's
    touched-line update and with it every parameter are those of the exact-size step.
The first step at an unseen capacity runs eagerly (library workspaces may not grow inside a capture), the next one is captured;
all graphs share one memory pool.  The palette distillation (style_encoder.py:160-173) runs once, eagerly, before step
`distill_step(iters, distill_palette_steps)`; it changes the active-base mask, a host argument of the palette kernels, so every
graph is dropped and recaptured.

Deviations from the reference: the jitter comes from Philox (include/laenerf.h lae_sample_edit_view), not torch's
device generator; with fewer than 16 views a 16-step group continues with further fresh permutations where the reference's
exhausted DataLoader raises StopIteration.  Out of scope, refused with NotImplementedError: the VGG style, TV, depth-discontinuity
and smooth-transition terms, preserve_color and intensity_weight.
"""
import math
import time

import numpy as np
import torch

from .. import _lib
from ..backend import style_backend as _backend
from ..trainer import bucket_capacity

__all__ = ["EditSet", "StyleTrainer", "jitter_numpy", "draw_schedule", "view_schedule", "capacity_for", "distill_step"]

GROUP = 16                          # steps per train_LAENeRF_step call (nerf/gui.py:1997-2026)
_JITTER_WORD3 = 2                   # Philox counter word 3 of the jitter draw (include/laenerf.h)


# ------------------------------------------------------------------------------------------------------------ host-side rules
def jitter_numpy(x_term, dirs, depth_factor, seed, step, rows=None):
    """numpy restatement of lae_sample_edit_view's jitter: x = x_term + ((u - 0.5) * depth_factor) * dirs in float32, u = (w >> 8)
    * 2^-24, w = Philox4x32-10 word 0 at counter (step, row, 0, 2).  x_term, dirs [K,3] are the view's rows; rows: their row numbers
    (default 0..K-1) -> [K,3] float32"""
    from ..data import _u32
    x_term = np.asarray(x_term, np.float32)
    dirs = np.asarray(dirs, np.float32)
    rows = np.arange(x_term.shape[0], dtype=np.uint64) if rows is None else np.asarray(rows, np.uint64)
    w = _u32(int(seed) & 0xFFFFFFFFFFFFFFFF, step, rows, 0, _JITTER_WORD3)
    u = (w >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    t = (u - np.float32(0.5)) * np.float32(depth_factor)
    return x_term + t[:, None] * dirs


def draw_schedule(gen, V, n_steps):
    """the view of each of ceil(n_steps / 16) * 16 steps: every 16-step group is the first 16 entries of a fresh torch.randperm(V,
    generator=gen) (the reference re-creates its shuffled DataLoader iterator at every 16-step call); with V < 16 the group continues
    with further fresh permutations (the reference raises StopIteration there) -> int32 [n]"""
    if V < 1:
        raise ValueError("draw_schedule: no views")
    out = []
    for _ in range(-(-int(n_steps) // GROUP)):
        group = []
        while len(group) < GROUP:
            group.extend(torch.randperm(V, generator=gen)[:GROUP - len(group)].tolist())
        out.extend(group)
    return np.asarray(out, dtype=np.int32)


def view_schedule(V, n_steps, seed=0):
    """draw_schedule from torch.Generator().manual_seed(seed): StyleTrainer's schedule for `seed`"""
    return draw_schedule(torch.Generator().manual_seed(int(seed)), V, n_steps)


def capacity_for(K, capacity="bucket"):
    """buffer rows of a step on a view of K points: 'exact' = K rounded up to 16 (the MLP tile); 'bucket' = K rounded up to 8 steps per
    octave (trainer.bucket_capacity with 16-row alignment: at most 12.5 % pad rows above 128 points)"""
    K = int(K)
    if K < 1:
        raise ValueError("capacity_for: a view has at least one point")
    if capacity == "exact":
        return -(-K // 16) * 16
    if capacity == "bucket":
        return bucket_capacity(K, 16)
    raise ValueError("capacity must be 'bucket' or 'exact'")


def distill_step(iters, distill_palette_steps):
    """the global step before which the palette distillation runs: the first multiple of 16 (a call boundary of the reference's
    16-step loop) greater than iters - distill_palette_steps, if it is < iters (nerf/gui.py:1997-2004); None: never (also for
    distill_palette_steps < 0, the reference's 'done' marker)"""
    if distill_palette_steps is None or distill_palette_steps < 0:
        return None
    s = max(0, ((int(iters) - int(distill_palette_steps)) // GROUP + 1) * GROUP)
    return s if s < int(iters) else None


# ------------------------------------------------------------------------------------------------------------------ the set
class EditSet:
    """The training views of the palette network, packed once: x_term, dirs, targets [sum K, 3] fp32, offsets [V] int64, counts [V]
    int32, depth_factor [V] fp32, a device step counter and a device view schedule (default: step mod V; StyleTrainer installs its
    own).  device='cpu' keeps the arrays on the host (loaders, tests); sample() needs the GPU."""

    def __init__(self, x_term, dirs, targets, counts, depth_factor, seed=0, device=None):
        device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        t = lambda a, dt: (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to(device, dt).contiguous()
        counts_h = np.asarray(counts.cpu() if torch.is_tensor(counts) else counts, dtype=np.int64).reshape(-1)
        if counts_h.size == 0 or (counts_h < 1).any() or counts_h.max() >= 2 ** 31:
            raise ValueError("EditSet: every view needs 1 .. 2^31 - 1 points")
        n = int(counts_h.sum())
        self.x_term, self.dirs, self.targets = t(x_term, torch.float32), t(dirs, torch.float32), t(targets, torch.float32)
        for name, a in (("x_term", self.x_term), ("dirs", self.dirs), ("targets", self.targets)):
            if tuple(a.shape) != (n, 3):
                raise ValueError(f"EditSet: {name} must be [sum(counts) = {n}, 3]")
        self.depth_factor = t(np.asarray(depth_factor.cpu() if torch.is_tensor(depth_factor) else depth_factor, np.float32).reshape(-1),
                              torch.float32)
        if self.depth_factor.numel() != counts_h.size:
            raise ValueError("EditSet: one depth_factor per view")
        self.counts_host = counts_h
        self.offsets_host = np.concatenate([[0], np.cumsum(counts_h)[:-1]]).astype(np.int64)
        self.counts = torch.from_numpy(counts_h.astype(np.int32)).to(device)
        self.offsets = torch.from_numpy(self.offsets_host).to(device)
        self.V = int(counts_h.size)
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.step = torch.zeros(1, dtype=torch.int64, device=device)
        self.set_schedule(np.arange(self.V, dtype=np.int32))
        self._out = {}

    @property
    def device(self):
        return self.x_term.device

    @classmethod
    def from_arrays(cls, x_term, dirs, targets, counts, depth_factor, **kw):
        return cls(x_term, dirs, targets, counts, depth_factor, **kw)

    @classmethod
    def from_views(cls, views, **kw):
        """the per-view dicts of extract_views / extract_view (x_term, dirs, targets, depth_factor; CPU or device tensors)"""
        views = list(views)
        if not views:
            raise ValueError("EditSet.from_views: no views")
        cat = lambda key: torch.cat([v[key].detach().float().reshape(-1, 3).cpu() for v in views])
        counts = [int(v["x_term"].shape[0]) for v in views]
        df = [float(v["depth_factor"]) for v in views]
        return cls(cat("x_term"), cat("dirs"), cat("targets"), counts, np.asarray(df, np.float32), **kw)

    def save(self, path):
        """one .npz of the packed arrays (the counterpart of the reference's --save/--load_edit_dataset)"""
        np.savez(path, x_term=self.x_term.cpu().numpy(), dirs=self.dirs.cpu().numpy(), targets=self.targets.cpu().numpy(),
                 counts=self.counts_host.astype(np.int32), depth_factor=self.depth_factor.cpu().numpy(), seed=np.uint64(self.seed))

    @classmethod
    def load(cls, path, device=None):
        with np.load(path) as z:
            return cls(z["x_term"], z["dirs"], z["targets"], z["counts"], z["depth_factor"], seed=int(z["seed"]), device=device)

    def set_schedule(self, views):
        """the device table the sampler reads at step s: views[s mod len(views)]"""
        v = np.asarray(views, dtype=np.int64).reshape(-1)
        if v.size == 0 or (v < 0).any() or (v >= self.V).any():
            raise ValueError(f"EditSet.set_schedule: view indices must lie in 0..{self.V - 1}")
        self.schedule_host = v.astype(np.int32)
        self.schedule = torch.from_numpy(self.schedule_host).to(self.device)

    def view_points(self, v):
        """the un-jittered x_term [K,3] of view v (a view of the packed array)"""
        o, k = int(self.offsets_host[v]), int(self.counts_host[v])
        return self.x_term[o:o + k]

    def view_arrays(self, v):
        """(x_term, dirs, targets) of view v, un-jittered"""
        o, k = int(self.offsets_host[v]), int(self.counts_host[v])
        return self.x_term[o:o + k], self.dirs[o:o + k], self.targets[o:o + k]

    def _buffers(self, cap):
        out = self._out.get(cap)
        if out is None:
            dev = self.device
            out = self._out[cap] = (torch.empty(cap, 3, dtype=torch.float32, device=dev), torch.empty(cap, 3, dtype=torch.float32, device=dev),
                                    torch.empty(cap, 3, dtype=torch.float32, device=dev), torch.empty(1, dtype=torch.int32, device=dev))
        return out

    @torch.no_grad()
    def sample(self, cap, step=None):
        """the view of the schedule at the device step counter -> (x, d, target [cap,3] fp32, m_dev [1] int32 = K) through
        lae_sample_edit_view; the counter is then advanced (capturable).  step=k sets the counter to k first.  cap must be a multiple
        of 4 (16 for the palette network) and >= the view's K, which is otherwise cut to cap rows.  The tensors are reused by the
        next call with the same cap."""
        cap = int(cap)
        if cap < 1 or cap % 4:
            raise ValueError("EditSet.sample: cap must be a positive multiple of 4")
        _lib.need_cuda(self.x_term)
        if step is not None:
            self.step.fill_(int(step))
        x, d, t, m = self._buffers(cap)
        _backend.sample_edit_view(self.x_term, self.dirs, self.targets, self.offsets, self.counts, self.depth_factor, self.schedule, cap,
                                  self.seed, self.step, x, d, t, m)
        return x, d, t, m


# -------------------------------------------------------------------------------------------------------------- the trainer
_REFUSED = ("style_weight", "tv_weight", "depth_disc_weight", "smooth_trans_weight", "intensity_weight")


def fused_step_loss(enc, x, d, target, m_dev, params, opt):
    """the loss of one step as StyleTrainer computes it: forward_train + MSE + weights_loss + offset_loss + palet_loss
    (nerf/utils.py:987-995) as one node over the first *m_dev rows of the [cap,3] buffers, scaled by opt's GradScaler"""
    with torch.autocast("cuda", dtype=torch.float16):
        loss, *_ = enc.forward_train_loss(x, d, target, params, opt, with_palet_loss=True, m_dev=m_dev)
    return loss


class StyleTrainer:
    """StyleTrainer(style_enc, edit_set, params, iters): trains the LAENeRF `style_enc` on the EditSet `edit_set` for the reference's
    `train_steps_style` = iters steps (more are allowed: train() is resumable and the schedule is extended).  `params` carries the
    loss weights (weight_loss_uniform, weight_loss_non_uniform, offset_loss, palette_loss_valid, palette_loss_distinct).
    Optimizer: FusedAdam over style_enc.get_params(lr) (palette 2 lr), betas (0.9, 0.999), eps 1e-8, with its GradScaler (.opt).
    graph=False runs the same steps eagerly; capacity 'bucket' / 'exact' (module docstring).
    Counters: captures (graphs captured), cache_misses (steps that found no graph for their capacity), steps_skipped (GradScaler)."""

    def __init__(self, style_enc, edit_set, params, iters, distill_palette_steps=1500, seed=0, graph=True, capacity="bucket", lr=1e-3):
        from ..optim import FusedAdam
        if capacity not in ("bucket", "exact"):
            raise ValueError("StyleTrainer: capacity must be 'bucket' or 'exact'")
        for name in _REFUSED:
            if float(getattr(params, name, 0) or 0) > 0:
                raise NotImplementedError(f"StyleTrainer: {name} > 0 is outside the palette network's point losses (DESIGN.md 4c)")
        if getattr(params, "preserve_color", False):
            raise NotImplementedError("StyleTrainer: preserve_color is not supported (DESIGN.md 4c)")
        if edit_set.device != style_enc.color_palette.device:
            raise ValueError("StyleTrainer: the edit set and the network must live on the same device")
        self.enc, self.es, self.params = style_enc, edit_set, params
        self.iters, self.graph, self.capacity = int(iters), bool(graph), capacity
        self.opt = FusedAdam(style_enc, param_groups=style_enc.get_params(lr), betas=(0.9, 0.999), eps=1e-8)
        self.gen = torch.Generator().manual_seed(int(seed))
        edit_set.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self._sched = draw_schedule(self.gen, edit_set.V, max(self.iters, 1))
        edit_set.set_schedule(self._sched)
        self.rec = torch.zeros(self._sched.size, 2, dtype=torch.float32, device=edit_set.device)     # per step: loss, mse
        self.s_d = distill_step(self.iters, distill_palette_steps)
        self.distilled = False
        self.distill_ms = None
        self.global_step = 0
        self.started = False
        self.graphs = {}
        self._pool = None
        self._warm = set()
        self.captures = self.cache_misses = 0
        self._hist = []

    def cap_of_step(self, s):
        """the buffer capacity of global step s"""
        return capacity_for(self.es.counts_host[self._sched[s]], self.capacity)

    # ------------------------------------------------------------------ one step
    def _step(self, cap):
        x, d, t, m = self.es.sample(cap)
        loss = fused_step_loss(self.enc, x, d, t, m, self.params, self.opt)
        self.opt.backward(loss)
        self.opt.step()
        with torch.no_grad():
            self.rec.index_copy_(0, self.es.step - 1, loss.terms[1:3].view(1, 2))

    def _graph_step(self, cap):
        g = self.graphs.get(cap)
        if g is None:
            self.cache_misses += 1
            if cap not in self._warm:
                # the encoder / MLP / loss workspaces may have to grow to cap rows, which is refused inside a capture: this step runs
                # eagerly (the same kernels, hence the same bits) and the next one at this capacity is captured
                self._step(cap)
                self._warm.add(cap)
                return
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, pool=self._pool):
                self._step(cap)
            if self._pool is None:
                self._pool = g.pool()
            self.graphs[cap] = g
            self.captures += 1
        g.replay()

    def _extend(self):
        """training past the schedule: more 16-step groups from the same generator (the table and the records are reallocated, so
        the graphs, which hold their addresses, are dropped)"""
        more = draw_schedule(self.gen, self.es.V, max(self._sched.size, GROUP))
        self._sched = np.concatenate([self._sched, more])
        self.es.set_schedule(self._sched)
        rec = torch.zeros(self._sched.size, 2, dtype=torch.float32, device=self.es.device)
        rec[:self.rec.shape[0]].copy_(self.rec)
        self.rec = rec
        self.graphs.clear()

    @torch.no_grad()
    def _distill(self):
        """distill_color_palettes on 10 views drawn from the trainer's generator, un-jittered (style_encoder.py:160-173), once"""
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        idx = torch.randint(0, self.es.V, (10,), generator=self.gen)
        xs = [self.es.view_points(v) for v in range(self.es.V)]
        with torch.autocast("cuda", dtype=torch.float16):
            self.enc.distill_color_palettes(xs, n=10, thresh=0.025, idx=idx)
        self.graphs.clear()                    # n_active / the active mask are host arguments of the captured palette kernels
        self.distilled = True
        torch.cuda.synchronize()
        self.distill_ms = (time.perf_counter() - t0) * 1e3

    def train(self, n_steps):
        """n_steps steps of the reference's loop; the palette distillation runs before global step s_d (once)"""
        if not self.started:
            self.es.set_schedule(self._sched)
            self.es.step.fill_(self.global_step)
            self.started = True
        self.enc.train()
        start = self.global_step
        for _ in range(int(n_steps)):
            s = self.global_step
            if self.s_d is not None and s >= self.s_d and not self.distilled:
                self._distill()
            if s >= self._sched.size:
                self._extend()
            cap = self.cap_of_step(s)
            if self.graph:
                self._graph_step(cap)
            else:
                self._step(cap)
            self.global_step += 1
        if self.global_step > start:
            self._hist.append(self.rec[start:self.global_step].cpu().numpy())        # the one host read of the call
        return self

    # ------------------------------------------------------------------ results
    def _records(self):
        return np.concatenate(self._hist) if self._hist else np.zeros((0, 2), np.float32)

    def losses(self):
        """per-step unscaled losses (MSE + weight + offset + palette terms, nerf/utils.py:990-995) as float32"""
        return self._records()[:, 0]

    def mse(self):
        """per-step MSE term"""
        return self._records()[:, 1]

    def group_psnr(self):
        """what the reference prints per 16-step call: 10 log10(1 / average loss) (nerf/utils.py:1041-1049), one value per complete
        group"""
        lo = self.losses().astype(np.float64)
        n = lo.size // GROUP
        return np.array([10.0 * math.log10(1.0 / lo[g * GROUP:(g + 1) * GROUP].mean()) for g in range(n)])

    @property
    def steps_skipped(self):
        """optimizer steps the GradScaler skipped (non-finite gradients)"""
        return self.opt.steps_skipped
