"""bench.py's plain line, --full and --dump-outputs, run in-process at a small size.

A plain run carries the headline figures and nothing that takes a run of its own; --full adds the
acting roofline and the step-kernel line (the CPU baselines, tens of seconds, are switched off here);
--dump-outputs writes the last timed step's arrays as float .npy files, the same names, shapes and
sampled rows on every run."""
import json
import os
import sys

import numpy as np
import pytest

SMALL = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--envs", "64", "--update-step", "8"]
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
OWN_RUNS = ("act_roofline", "step_kernel", "cpu_baseline", "cpu_baseline_e1")


def _bench(monkeypatch, capsys, args):
    import bench

    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py"] + args)
    bench.main()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_full_and_dump_options_parse_without_a_gpu(monkeypatch, capsys, tmp_path):
    d = _bench(monkeypatch, capsys, ["--stub", "--full", "--dump-outputs", str(tmp_path / "out")])
    assert d["metric"] == "launcher stub" and d["n_gpus"] == 1
    with pytest.raises(SystemExit):
        _bench(monkeypatch, capsys, ["--stub", "--steps", "0"])


@pytest.mark.gpu
def test_plain_line_and_dumped_outputs(monkeypatch, capsys, tmp_path):
    import bench

    monkeypatch.setattr(bench, "DUMP_ROWS", 100)  # 8 rounds x 64 replicas = 512 rows: sampled
    runs = []
    for name in ("a", "b"):
        d = _bench(monkeypatch, capsys, SMALL + ["--dump-outputs", str(tmp_path / name)])
        assert all(k in d for k in HEADLINE) and not any(k in d for k in OWN_RUNS)
        assert d["steps"] == 2 and d["higher_is_better"] is True and d["unit"] == "agent-env-steps/s"
        # value = agents x replicas x rounds of the timed steps / their wall time
        assert d["value"] == pytest.approx(64 * 8 * 8 / (d["ms_per_step"] / 1e3), rel=1e-9)
        files = {f: np.load(tmp_path / name / f) for f in sorted(os.listdir(tmp_path / name))}
        assert all(f.endswith(".npy") for f in files)
        assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in files.values())
        assert sum(a.nbytes for a in files.values()) <= 64 << 20
        runs.append(files)
    a, b = runs
    for unit in ("acceptor", "offer", "price"):
        assert "loss_%s.npy" % unit in a and "weights_%s_w1.npy" % unit in a
        assert a["rollout_%s_actions.npy" % unit].shape[0] == 100  # the sampled (round, replica) rows
    assert a["next_offer_obs.npy"].shape[0] == 64 and a["agent_reward.npy"].shape == (64, 8)
    assert {k: v.shape for k, v in a.items()} == {k: v.shape for k, v in b.items()}
    assert np.array_equal(a["rows_512.npy"], b["rows_512.npy"])
    assert len(np.unique(a["rows_512.npy"])) == 100 and a["rows_512.npy"].max() < 512


@pytest.mark.gpu
def test_full_adds_the_runs_of_their_own(monkeypatch, capsys):
    d = _bench(monkeypatch, capsys, SMALL + ["--full", "--no-cpu-baseline"])
    assert all(k in d for k in HEADLINE)
    assert d["act_roofline"]["avg_launch_us"] > 0
    assert d["step_kernel"]["timed_rounds"] == 2000 and d["step_kernel"]["value"] > 0
    assert "cpu_baseline" not in d
