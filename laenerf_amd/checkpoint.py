"""Checkpoint files: the host side of Trainer.save_checkpoint / load_checkpoint and StyleTrainer's (pure host code, no GPU needed).

The file is the reference Trainer's `ngp_epXXXX.pth` (nerf/utils.py:1626-1753): a dict with epoch, global_step, stats, mean_count,
mean_density, model and, when `full`, optimizer (torch.optim.Adam's layout), lr_scheduler (a LambdaLR-shaped dict), scaler
(torch.cuda.amp.GradScaler's layout) and ema (torch_ema's layout).  One more key, `laenerf_amd`, holds what a bit-exact resume needs
beyond that (laenerf_amd.trainer).  A file holds only tensors and plain Python containers and scalars, so
`torch.load(path, weights_only=True)` reads it; that is how read_checkpoint reads unless `trusted=True`.
"""
import glob
import os
import tempfile

import torch

__all__ = ["FORMAT", "KEY", "atomic_save", "checkpoint_name", "latest_checkpoint", "resolve_path", "rotate", "read_checkpoint",
           "new_stats", "scaler_to_reference", "scaler_from_reference", "scheduler_to_reference", "scheduler_from_reference",
           "check_config", "shapes_of", "format_differences"]

FORMAT = 1                      # the layout of the `laenerf_amd` entry
KEY = "laenerf_amd"


# ---------------------------------------------------------------------------------------------------------------- files
def atomic_save(obj, path):
    """torch.save(obj) to a temporary name in path's directory, then os.replace: a failure while writing leaves no partial file and
    an older file of the same name intact"""
    path = os.fspath(path)
    directory = os.path.dirname(os.path.abspath(path))
    os.makedirs(directory, exist_ok=True)
    fd, tmp = tempfile.mkstemp(prefix=os.path.basename(path) + ".", suffix=".tmp", dir=directory)
    try:
        with os.fdopen(fd, "wb") as f:
            torch.save(obj, f)
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, path)
    except BaseException:
        if os.path.exists(tmp):
            os.remove(tmp)
        raise
    return path


def checkpoint_name(name, epoch):
    """the reference's file name of an epoch's checkpoint (nerf/utils.py:1629)"""
    return f"{name}_ep{int(epoch):04d}.pth"


def latest_checkpoint(directory, name="ngp"):
    """the reference's rule (nerf/utils.py:1695-1697): the last of sorted(glob('{directory}/{name}_ep*.pth')); None when there is none"""
    found = sorted(glob.glob(os.path.join(glob.escape(os.fspath(directory)), f"{glob.escape(name)}_ep*.pth")))
    return found[-1] if found else None


def resolve_path(path_or_dir, name="ngp", epoch=None, best=False):
    """where save_checkpoint writes: a `.pth` path as it is; otherwise a directory, with checkpoint_name(name, epoch) -- or
    `{name}.pth` for the best checkpoint, the reference's best_path"""
    p = os.fspath(path_or_dir)
    if p.endswith(".pth"):
        return p, False
    return os.path.join(p, f"{name}.pth" if best else checkpoint_name(name, epoch)), True


def rotate(stats, path, max_keep_ckpt=2):
    """nerf/utils.py:1659-1665: `path` joins stats['checkpoints'], which keeps at most max_keep_ckpt paths; the oldest ones leave the
    list and the disk -> the removed paths.  Call it before the file is written: the file then lists itself, like the reference's."""
    ckpts = stats.setdefault("checkpoints", [])
    if path in ckpts:
        ckpts.remove(path)
    ckpts.append(path)
    removed = []
    while len(ckpts) > max(int(max_keep_ckpt), 1):
        old = ckpts.pop(0)
        removed.append(old)
        if os.path.exists(old):
            os.remove(old)
    return removed


def read_checkpoint(path, trusted=False):
    """the file's dict, on the host.  trusted=True: a full unpickle, for reference files that carry other objects -- only for files
    whose origin is known"""
    return torch.load(path, map_location="cpu", weights_only=not trusted)


def new_stats():
    """the reference Trainer's stats (nerf/utils.py:436-442)"""
    return {"loss": [], "valid_loss": [], "results": [], "checkpoints": [], "best_result": None}


# ------------------------------------------------------------------------------------------------------------ converters
def scaler_to_reference(scale, growth_tracker, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000):
    """torch.cuda.amp.GradScaler.state_dict() of an enabled scaler"""
    return {"scale": float(scale), "growth_factor": float(growth_factor), "backoff_factor": float(backoff_factor),
            "growth_interval": int(growth_interval), "_growth_tracker": int(growth_tracker)}


def scaler_from_reference(sd):
    """-> dict scale, growth_tracker, growth_factor, backoff_factor, growth_interval, or None for the empty dict of a disabled
    GradScaler.  FusedAdam's own short form {scale, growth_tracker} is read too."""
    if not sd:
        return None
    if "scale" not in sd:
        raise ValueError("checkpoint: a scaler entry without 'scale'")
    tracker = sd["_growth_tracker"] if "_growth_tracker" in sd else sd.get("growth_tracker", 0)
    out = {"scale": float(sd["scale"]), "growth_tracker": int(tracker)}
    for k, cast in (("growth_factor", float), ("backoff_factor", float), ("growth_interval", int)):
        if k in sd:
            out[k] = cast(sd[k])
    return out


def scheduler_to_reference(last_epoch, base_lrs, iters):
    """the LambdaLR.state_dict() of the reference's per-step schedule lr * 0.1 ** min(it / iters, 1) (main_nerf.py:239-245) after
    `last_epoch` scheduler steps, one base rate per parameter group.  lr_lambdas holds None per group, as LambdaLR writes for a
    function that is no callable object."""
    last_epoch = int(last_epoch)
    base = [float(b) for b in base_lrs]
    f = 0.1 ** min(last_epoch / int(iters), 1.0)
    return {"base_lrs": base, "last_epoch": last_epoch, "verbose": False, "_step_count": last_epoch + 1,
            "_get_lr_called_within_step": False, "_last_lr": [b * f for b in base], "lr_lambdas": [None] * len(base)}


def scheduler_from_reference(sd):
    """-> dict last_epoch (int), base_lrs, last_lr (lists of float) from a LambdaLR-shaped dict; missing lists come back empty"""
    if "last_epoch" not in sd:
        raise ValueError("checkpoint: an lr_scheduler entry without 'last_epoch'")
    return {"last_epoch": int(sd["last_epoch"]), "base_lrs": [float(b) for b in sd.get("base_lrs", [])],
            "last_lr": [float(b) for b in sd.get("_last_lr", [])]}


# ------------------------------------------------------------------------------------------------------------ config
def _plain(v):
    if isinstance(v, (tuple, list)):
        return [_plain(x) for x in v]
    if isinstance(v, torch.Size):
        return [int(x) for x in v]
    return v


def _flatten(d, prefix=""):
    out = {}
    for k, v in d.items():
        if isinstance(v, dict):
            out.update(_flatten(v, f"{prefix}{k}."))
        else:
            out[f"{prefix}{k}"] = _plain(v)
    return out


def _same(a, b):
    if isinstance(a, bool) or isinstance(b, bool) or a is None or b is None:
        return type(a) is type(b) and a == b
    return a == b


_MISSING = "<missing>"


def check_config(saved, current):
    """the fields that differ between two configurations (dicts, possibly nested: nested names are joined with dots; tuples count
    as lists) -> [(name, saved value, current value)] in sorted name order; a field only one side has shows '<missing>' on the other"""
    a, b = _flatten(saved), _flatten(current)
    return [(k, a.get(k, _MISSING), b.get(k, _MISSING)) for k in sorted(set(a) | set(b))
            if k not in a or k not in b or not _same(a[k], b[k])]


def shapes_of(tensors, prefix=""):
    """{prefix + name: [shape]} of a dict (or a list, named by index) of tensors"""
    items = tensors.items() if isinstance(tensors, dict) else enumerate(tensors)
    return {f"{prefix}{k}": [int(x) for x in v.shape] for k, v in items if torch.is_tensor(v)}


def format_differences(diffs):
    return "; ".join(f"{n}: saved {s!r}, current {c!r}" for n, s, c in diffs)
