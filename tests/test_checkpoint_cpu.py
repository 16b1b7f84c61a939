"""laenerf_amd.checkpoint: the host side of the checkpoint files (no GPU)."""
import os

import pytest
import torch

from laenerf_amd import checkpoint as C


class _Opt:                                                               # the reference's files may carry such objects
    pass


def test_atomic_save_writes_and_replaces(tmp_path):
    p = str(tmp_path / "sub" / "a.pth")                                   # the directory is created
    assert C.atomic_save({"x": torch.arange(3)}, p) == p
    C.atomic_save({"x": torch.arange(4)}, p)
    assert torch.equal(torch.load(p, weights_only=True)["x"], torch.arange(4))
    assert os.listdir(tmp_path / "sub") == ["a.pth"]


def test_atomic_save_failure_leaves_no_partial_file(tmp_path, monkeypatch):
    real = torch.save

    def broken(obj, f, *a, **kw):
        f.write(b"half a file")                                          # some bytes reach the temporary file, then the write fails
        f.flush()
        raise OSError("disk full")

    fresh, old = str(tmp_path / "fresh.pth"), str(tmp_path / "old.pth")
    real({"x": torch.arange(5)}, old)
    before = open(old, "rb").read()
    monkeypatch.setattr(torch, "save", broken)
    for p in (fresh, old):
        with pytest.raises(OSError, match="disk full"):
            C.atomic_save({"x": torch.zeros(100)}, p)
    monkeypatch.setattr(torch, "save", real)
    assert sorted(os.listdir(tmp_path)) == ["old.pth"]                    # no fresh.pth, no temporary file
    assert open(old, "rb").read() == before and torch.equal(torch.load(old, weights_only=True)["x"], torch.arange(5))


def test_names_and_latest(tmp_path):
    assert C.checkpoint_name("ngp", 7) == "ngp_ep0007.pth" and C.checkpoint_name("run", 12345) == "run_ep12345.pth"
    assert C.latest_checkpoint(str(tmp_path)) is None
    for f in ("ngp_ep0002.pth", "ngp_ep0010.pth", "ngp_ep0009.pth", "ngp.pth", "other_ep0099.pth", "ngp_ep0011.txt", "ngp_ep0003.pth.tmp"):
        (tmp_path / f).write_bytes(b"")
    assert C.latest_checkpoint(str(tmp_path)) == str(tmp_path / "ngp_ep0010.pth")
    assert C.latest_checkpoint(str(tmp_path), "other") == str(tmp_path / "other_ep0099.pth")
    assert C.latest_checkpoint(str(tmp_path), "none") is None
    assert C.resolve_path(str(tmp_path / "x.pth"), "ngp", 3) == (str(tmp_path / "x.pth"), False)
    assert C.resolve_path(str(tmp_path), "ngp", 3) == (str(tmp_path / "ngp_ep0003.pth"), True)
    assert C.resolve_path(str(tmp_path), "ngp", 3, best=True) == (str(tmp_path / "ngp.pth"), True)


def test_rotation_keeps_the_newest(tmp_path):
    stats = C.new_stats()
    assert stats == {"loss": [], "valid_loss": [], "results": [], "checkpoints": [], "best_result": None}
    paths = [str(tmp_path / C.checkpoint_name("ngp", e)) for e in range(5)]
    for i, p in enumerate(paths):
        removed = C.rotate(stats, p)                                     # default: max_keep_ckpt = 2
        C.atomic_save({"epoch": i}, p)
        assert removed == ([paths[i - 2]] if i >= 2 else [])
        assert stats["checkpoints"] == paths[max(0, i - 1):i + 1]
        assert sorted(os.listdir(tmp_path)) == [os.path.basename(q) for q in paths[max(0, i - 1):i + 1]]
    assert C.rotate(stats, paths[4]) == [] and stats["checkpoints"] == paths[3:]      # the same path again is listed once
    stats3 = C.new_stats()
    for p in paths:
        C.rotate(stats3, p, max_keep_ckpt=3)
    assert stats3["checkpoints"] == paths[2:]                            # files that are gone already are no error


def test_scaler_converter_round_trip():
    # torch.cuda.amp.GradScaler.state_dict() of an enabled scaler (torch/amp/grad_scaler.py), and of GradScaler(enabled=False)
    enabled = {"scale": 32768.0, "growth_factor": 2.0, "backoff_factor": 0.5, "growth_interval": 2000, "_growth_tracker": 123}
    disabled = torch.amp.GradScaler("cpu", enabled=False).state_dict()
    assert disabled == {} and C.scaler_from_reference(disabled) is None
    got = C.scaler_from_reference(enabled)
    assert got == {"scale": 32768.0, "growth_tracker": 123, "growth_factor": 2.0, "backoff_factor": 0.5, "growth_interval": 2000}
    assert C.scaler_to_reference(got["scale"], got["growth_tracker"], got["growth_factor"], got["backoff_factor"],
                                 got["growth_interval"]) == enabled
    assert C.scaler_from_reference({"scale": 8.0, "growth_tracker": 3}) == {"scale": 8.0, "growth_tracker": 3}    # FusedAdam's short form
    with pytest.raises(ValueError):
        C.scaler_from_reference({"growth_factor": 2.0})


def test_scheduler_converter_round_trip():
    iters, lr = 50, 1e-2
    params = [torch.nn.Parameter(torch.zeros(1)) for _ in range(2)]
    opt = torch.optim.Adam([{"params": [params[0]], "lr": lr}, {"params": [params[1]], "lr": 2 * lr}])
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda it: 0.1 ** min(it / iters, 1))
    for _ in range(7):
        opt.step()
        sched.step()
    real = sched.state_dict()
    got = C.scheduler_from_reference(real)
    assert got["last_epoch"] == 7 and got["base_lrs"] == [lr, 2 * lr] and got["last_lr"] == pytest.approx(real["_last_lr"], rel=1e-15)
    ours = C.scheduler_to_reference(got["last_epoch"], got["base_lrs"], iters)
    for k in ("last_epoch", "base_lrs", "_step_count", "lr_lambdas"):
        assert ours[k] == real[k], k
    assert ours["_last_lr"] == pytest.approx(real["_last_lr"], rel=1e-15)
    assert C.scheduler_from_reference(ours) == {**got, "last_lr": ours["_last_lr"]}
    # a real LambdaLR takes the dict
    opt2 = torch.optim.Adam([{"params": [params[0]], "lr": lr}, {"params": [params[1]], "lr": 2 * lr}])
    sched2 = torch.optim.lr_scheduler.LambdaLR(opt2, lambda it: 0.1 ** min(it / iters, 1))
    sched2.load_state_dict(ours)
    opt2.step()
    sched2.step()
    opt.step()
    sched.step()
    assert sched2.last_epoch == 8 and sched2.get_last_lr() == pytest.approx(sched.get_last_lr(), rel=1e-15)
    assert C.scheduler_to_reference(200, [lr], iters)["_last_lr"] == pytest.approx([lr * 0.1])      # past the horizon: the floor
    with pytest.raises(ValueError):
        C.scheduler_from_reference({"base_lrs": [lr]})


def test_check_config_reports_exactly_the_differing_fields():
    saved = {"iters": 400, "lr": [0.01, 0.01], "num_rays": 2048, "error_map": None, "depth_grad": True, "dt_gamma": 0.0,
             "data": {"n_img": 6, "H": 48, "mode": "image"}, "renderer": {"bound": 1, "grid_size": 128},
             "shapes": {"model.encoder.embeddings": [1000, 2], "model.density_grid": [1, 8]}}
    same = {"iters": 400, "lr": (0.01, 0.01), "num_rays": 2048, "error_map": None, "depth_grad": True, "dt_gamma": 0,
            "data": {"n_img": 6, "H": 48, "mode": "image"}, "renderer": {"bound": 1.0, "grid_size": 128},
            "shapes": {"model.encoder.embeddings": torch.Size([1000, 2]), "model.density_grid": (1, 8)}}
    assert C.check_config(saved, saved) == [] and C.check_config(saved, same) == []
    cur = {"iters": 400, "lr": [0.01, 0.02], "num_rays": 4096, "error_map": "ema", "depth_grad": 1, "dt_gamma": 0.0,
           "data": {"n_img": 6, "H": 40, "mode": "image"}, "renderer": {"bound": 1, "grid_size": 128, "min_near": 0.2},
           "shapes": {"model.encoder.embeddings": [500, 2]}}
    diffs = C.check_config(saved, cur)
    assert diffs == [("data.H", 48, 40), ("depth_grad", True, 1), ("error_map", None, "ema"), ("lr", [0.01, 0.01], [0.01, 0.02]),
                     ("num_rays", 2048, 4096), ("renderer.min_near", "<missing>", 0.2), ("shapes.model.density_grid", [1, 8], "<missing>"),
                     ("shapes.model.encoder.embeddings", [1000, 2], [500, 2])]
    text = C.format_differences(diffs)
    assert "num_rays: saved 2048, current 4096" in text and "shapes.model.encoder.embeddings" in text


def test_files_read_with_weights_only(tmp_path):
    """a file of tensors and plain containers reads with weights_only=True, the default of read_checkpoint; another object needs
    trusted=True"""
    p = str(tmp_path / "ok.pth")
    C.atomic_save({"stats": C.new_stats(), "model": {"w": torch.ones(2, 2)}, C.KEY: {"format": C.FORMAT, "lr": [0.01], "mode": None}}, p)
    ck = C.read_checkpoint(p)
    assert ck[C.KEY]["format"] == C.FORMAT and torch.equal(ck["model"]["w"], torch.ones(2, 2))

    q = str(tmp_path / "obj.pth")
    C.atomic_save({"model": {}, "opt": _Opt()}, q)
    with pytest.raises(Exception):
        C.read_checkpoint(q)
    assert isinstance(C.read_checkpoint(q, trusted=True)["opt"], _Opt)
