"""bench.py's single-process command line: --dump-outputs, --full, the
result line, and the MIOpen find-db seeding (all on CPU)."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run_bench(*extra):
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    out = subprocess.run(
        [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1",
         "--steps", "2", "--warmup", "1", "--batch-size", "4",
         "--image", "32", *extra],
        cwd=REPO, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, f"stdout:\n{out.stdout}\nstderr:\n{out.stderr}"
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


@pytest.fixture(scope="module")
def two_runs(tmp_path_factory):
    a = tmp_path_factory.mktemp("dump_a")
    b = tmp_path_factory.mktemp("dump_b")
    res_a = _run_bench("--dump-outputs", str(a))
    res_b = _run_bench("--dump-outputs", str(b), "--full")
    return (a, res_a), (b, res_b)


def test_result_line_fields(two_runs):
    for _, res in two_runs:
        assert res["metric"] == "train_images_per_sec"
        assert res["unit"] == "images/s"
        assert res["higher_is_better"] is True
        assert res["dtype"] == "fp32"
        assert res["steps"] == 2 and res["warmup"] == 1
        assert res["ms_per_step"] > 0


def test_steps_sets_the_timed_steps(monkeypatch, capsys):
    """--steps N: exactly N training steps run between the two clock
    readings (W warm-up steps before the first), and ms_per_step / value
    are that interval divided by N."""
    import bench
    from bdbnn_amd.engine import Trainer

    calls = []
    real = Trainer._step_losses

    def counted(self, *a, **k):
        calls.append(1)
        return real(self, *a, **k)

    class Clock:
        readings = []

        @classmethod
        def perf_counter(cls):
            cls.readings.append(len(calls))
            return 6.0 * (len(cls.readings) - 1)  # 0 s, then 6 s

    monkeypatch.setattr(Trainer, "_step_losses", counted)
    monkeypatch.setattr(bench, "time", Clock)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(sys, "argv", [
        "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "2",
        "--batch-size", "4", "--image", "32"])
    bench.main()
    assert Clock.readings == [2, 5]
    res = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert res["steps"] == 3 and res["warmup"] == 2
    assert res["ms_per_step"] == pytest.approx(2000.0)
    assert res["value"] == pytest.approx(4 * 3 / 6.0)


def test_dump_outputs_written_and_reproducible(two_runs):
    (a, _), (b, _) = two_runs
    names = sorted(os.listdir(a))
    assert names == ["ce.npy", "kurt.npy", "logits_std.npy", "loss.npy",
                     "update_norm.npy"]
    assert sorted(os.listdir(b)) == names
    total = 0
    for n in names:
        x, y = np.load(a / n), np.load(b / n)
        assert x.dtype == np.float32
        assert np.isfinite(x).all()
        # same arguments -> same seeded weights and inputs; the CPU path is
        # deterministic, so here the outputs match exactly
        np.testing.assert_array_equal(x, y)
        total += x.nbytes
    assert total <= 64 * 2**20
    loss, ce, kurt = (float(np.load(a / f"{n}.npy"))
                      for n in ("loss", "ce", "kurt"))
    assert loss == pytest.approx(ce + kurt, rel=1e-5)
    # the optimizer moved the weights, and the dump shows it
    assert float(np.load(a / "update_norm.npy")) > 0
    assert float(np.load(a / "logits_std.npy")) > 0


def _main_dump(monkeypatch, out_dir):
    import bench
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(sys, "argv", [
        "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1",
        "--batch-size", "4", "--image", "32", "--dump-outputs", str(out_dir)])
    bench.main()
    return {n[:-4]: float(np.load(out_dir / n)) for n in os.listdir(out_dir)}


def test_dump_depends_on_backward_and_optimizer(tmp_path, monkeypatch,
                                                capsys):
    """The dumped figures must move when the update is broken: with the
    optimizer step disabled the weights stay at their seeded values, and
    update_norm, kurt and the losses all show it."""
    from bdbnn_amd.engine import Trainer
    (tmp_path / "ok").mkdir()
    (tmp_path / "frozen").mkdir()
    ok = _main_dump(monkeypatch, tmp_path / "ok")

    init = Trainer.__init__

    def frozen_init(self, *a, **k):
        init(self, *a, **k)
        self.optimizer.step = lambda *a, **k: None

    monkeypatch.setattr(Trainer, "__init__", frozen_init)
    frozen = _main_dump(monkeypatch, tmp_path / "frozen")
    capsys.readouterr()
    assert frozen["update_norm"] == 0.0 and ok["update_norm"] > 0.0
    for name in ("kurt", "ce", "loss", "logits_std"):
        assert ok[name] != frozen[name], name


def test_dump_budget_is_enforced(tmp_path, monkeypatch):
    import torch
    import bench
    monkeypatch.setattr(bench, "_DUMP_MAX_BYTES", 1024)
    with pytest.raises(ValueError):
        bench._dump_outputs(str(tmp_path), {"a": torch.zeros(200),
                                            "b": torch.zeros(200)})


def test_dump_sample_of_large_output_is_fixed(tmp_path):
    import torch
    import bench
    n = bench._DUMP_MAX_ELEMS + 1000
    t = torch.arange(n, dtype=torch.float32)
    bench._dump_outputs(str(tmp_path / "a"), {"big": t})
    bench._dump_outputs(str(tmp_path / "b"), {"big": t})
    x = np.load(tmp_path / "a" / "big.npy")
    assert x.shape == (bench._DUMP_MAX_ELEMS,)
    np.testing.assert_array_equal(x, np.load(tmp_path / "b" / "big.npy"))
    assert (np.diff(x) > 0).all()  # distinct elements of the source
    assert x[0] == 0 and x[-1] == n - 1  # spread over the whole array


def test_seed_find_db_merges_without_replacing(tmp_path, monkeypatch):
    import bench
    src = os.path.join(REPO, "benchmarks", "miopen_find_db")
    names = [n for n in os.listdir(src) if n.endswith(".ufdb.txt")]
    assert names, "recorded find-db missing"
    with open(os.path.join(src, names[0])) as f:
        recorded = f.read().splitlines()
    key0 = recorded[0].split("=", 1)[0]
    # the user already has one of the keys (own value) and a foreign one,
    # in a file without a trailing newline
    dst = tmp_path / "db"
    dst.mkdir()
    (dst / names[0]).write_text(f"{key0}=mine\nother-key=theirs")
    monkeypatch.setenv("MIOPEN_USER_DB_PATH", str(dst))
    bench._seed_miopen_find_db()
    once = (dst / names[0]).read_text()
    lines = once.splitlines()
    assert f"{key0}=mine" in lines and "other-key=theirs" in lines
    assert set(recorded[1:]) <= set(lines)
    assert recorded[0] not in lines
    assert len(lines) == len(recorded) + 1
    bench._seed_miopen_find_db()  # idempotent
    assert (dst / names[0]).read_text() == once


def test_seed_find_db_warns_when_nothing_matches(tmp_path, monkeypatch,
                                                 capsys):
    import bench
    src = os.path.join(REPO, "benchmarks", "miopen_find_db")
    name = [n for n in os.listdir(src) if n.endswith(".ufdb.txt")][0]
    monkeypatch.setenv("MIOPEN_USER_DB_PATH", str(tmp_path))
    bench._seed_miopen_find_db(name[:name.index(".HIP.") + 8])
    assert "no recorded MIOpen find-db" not in capsys.readouterr().err
    bench._seed_miopen_find_db("gfx000ff.HIP.9_9_9_")
    assert "no recorded MIOpen find-db for gfx000ff" in capsys.readouterr().err
