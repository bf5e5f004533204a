"""bench.py's command line without a GPU: a plain run goes through set-up, warm-up, the timed steps, --dump-outputs and the
result line and nothing else; --full adds bench.full_figures (check step, device-resident steps, roofline, runner, CPU
baseline) to the same line.  The engines and the pipeline are replaced by host-side stand-ins that count their calls."""
import importlib
import json
import sys

import numpy as np
import pytest
import torch

HEADLINE_KEYS = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


class _FakePipeline:
    calls = None

    def __init__(self, det, seg, overlap=True):
        pass

    @staticmethod
    def pinned_like(imgs):
        return list(imgs)

    def submit_host(self, host, top_n=None):
        _FakePipeline.calls.append("submit")
        return len(host), top_n

    def collect_host(self, ticket):
        _FakePipeline.calls.append("collect")
        n, k = ticket
        return [(np.zeros((k, 4)), np.ones(k), np.zeros((k, 4), np.float32), np.ones((k, 1024, 1024), np.uint8))
                for _ in range(n)]

    def __getattr__(self, name):           # upload / run_uploaded: only full_figures may reach for them
        raise AssertionError(f"pipeline.{name} used by a plain run")


@pytest.fixture
def bench(monkeypatch):
    bench = importlib.import_module("bench")
    from inklayer_amd import pipeline
    _FakePipeline.calls = []
    monkeypatch.setattr(pipeline, "InkLayerPipeline", _FakePipeline)
    monkeypatch.setattr(bench, "build_engines", lambda dev, rank, world, batch: (None, None, 0.0))
    monkeypatch.setattr(torch.cuda, "set_device", lambda *a, **k: None)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    for leg in ("cpu_baseline", "runner_leg"):
        monkeypatch.setattr(bench, leg, lambda *a, **k: (_ for _ in ()).throw(AssertionError("secondary leg run")))
    for var in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(var, raising=False)
    return bench


def _run(bench, monkeypatch, capsys, *flags):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "2", "--batch", "2",
                                      "--boxes", "1", *flags])
    bench.main()
    lines = capsys.readouterr().out.splitlines()
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def test_plain_run_does_only_what_the_headline_needs(bench, monkeypatch, capsys, tmp_path):
    monkeypatch.setattr(bench, "full_figures", lambda *a, **k: (_ for _ in ()).throw(AssertionError("--full leg run")))
    out = _run(bench, monkeypatch, capsys, "--dump-outputs", str(tmp_path / "dump"))
    assert _FakePipeline.calls == ["submit", "submit", "collect", "collect"] \
        + ["submit", "submit", "collect", "submit", "collect", "collect"]       # 2 warm-up + 3 timed steps, no more
    assert all(k in out for k in HEADLINE_KEYS)
    assert out["unit"] == "sketches/s" and out["higher_is_better"] is True and out["steps"] == 3 and out["warmup"] == 2
    assert out["value"] == pytest.approx(2 * 1000.0 / out["ms_per_step"])
    for moved in ("timed_step_equals_synchronous_step", "device_resident", "roofline", "attention", "runner",
                  "cpu_baseline"):
        assert moved not in out
    assert sorted(p.name for p in (tmp_path / "dump").iterdir()) == sorted(
        n + ".npy" for n in ("boxes_per_sketch", "boxes_xyxy_norm", "scores", "boxes_pixel", "mask_pixel_counts",
                             "masks_sample_index", "masks_sample"))
    assert np.array_equal(np.load(tmp_path / "dump" / "mask_pixel_counts.npy"), np.full(2, 1024.0 * 1024.0))


def test_full_adds_the_secondary_figures_to_the_same_line(bench, monkeypatch, capsys):
    seen = {}

    def fake_full(args, pipe, det, seg, imgs, host, res, rank, world, dev, dt):
        seen["steps_before"] = list(_FakePipeline.calls)
        seen["res"], seen["dt"] = res, dt
        return {"timed_step_equals_synchronous_step": True, "roofline": {"frac": 0.5}}

    monkeypatch.setattr(bench, "full_figures", fake_full)
    out = _run(bench, monkeypatch, capsys, "--full", "--no-runner", "--no-cpu-baseline")
    assert seen["steps_before"].count("submit") == 5 and len(seen["res"]) == 2          # after the timed region
    assert out["timed_step_equals_synchronous_step"] is True and out["roofline"] == {"frac": 0.5}
    assert all(k in out for k in HEADLINE_KEYS)
    assert out["ms_per_step"] == pytest.approx(seen["dt"] / 3 * 1e3)
