"""bench.py's command line: a plain run is the headline only, --full switches the
rest on, --dump-outputs writes the MSM result as exact float64 limb arrays."""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def _parse(bench, monkeypatch, argv):
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    return bench.parse()


def test_plain_run_is_not_full(monkeypatch):
    bench = _bench()
    a = _parse(bench, monkeypatch, ["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.gpus, a.steps, a.warmup) == (1, 7, 2)
    assert a.full is False and a.dump_outputs is None
    a = _parse(bench, monkeypatch, ["--full", "--no-secondary", "--dump-outputs", "somewhere"])
    assert a.full is True and a.no_secondary is True and a.dump_outputs == "somewhere"


def test_dump_outputs_round_trips_the_bytes(tmp_path):
    bench = _bench()
    rng = np.random.default_rng(1)
    # random limbs, then every limb 2^32 - 1: all exact in float64
    for i, aff in enumerate((rng.integers(0, 256, 64, dtype=np.uint8).tobytes(), b"\xff" * 64)):
        d = tmp_path / str(i) / "dir"
        bench.dump_outputs(str(d), aff)
        assert os.listdir(d) == ["msm_affine.npy"]
        a = np.load(d / "msm_affine.npy")
        assert a.dtype == np.float64 and a.shape == (16,)
        assert a.astype("<u4").tobytes() == aff
