"""bench.py's launcher decision (the driver's `python bench.py --gpus N` shape and its torchrun shape): with no
launcher and N > 1 the bench starts one worker per GPU itself; under a launcher WORLD_SIZE must equal --gpus."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


@pytest.mark.parametrize("gpus,env,plan", [
    (1, {}, "run"),
    (2, {}, "spawn"),
    (8, {}, "spawn"),
    (8, {"WORLD_SIZE": "8"}, "run"),
    (1, {"WORLD_SIZE": "1"}, "run"),
    (2, {"WORLD_SIZE": "1"}, "mismatch"),
    (1, {"WORLD_SIZE": "4"}, "mismatch"),
    (0, {}, "mismatch"),
])
def test_launch_plan(gpus, env, plan):
    assert bench.launch_plan(gpus, env) == plan


def test_spawn_command_shape(monkeypatch):
    seen = {}

    class R:
        returncode = 7

    def fake_run(cmd, *a, **k):
        seen["cmd"] = cmd
        return R()

    monkeypatch.setattr(subprocess, "run", fake_run)
    rc = bench.spawn_workers(4, ["--gpus", "4", "--steps", "2"])
    assert rc == 7
    cmd = seen["cmd"]
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert "--nproc-per-node=4" in cmd and "127.0.0.1" in cmd
    assert cmd[-4:] == ["--gpus", "4", "--steps", "2"]
    assert os.path.basename(cmd[-5]) == "bench.py"


def test_mismatch_exits_nonzero_before_any_gpu_call():
    env = dict(os.environ, WORLD_SIZE="3", RANK="0", LOCAL_RANK="0")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2"], env=env,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 2
    assert "WORLD_SIZE=3" in p.stderr


def test_profile_order_is_by_round_then_tag_length():
    """profiles/ summaries are picked newest-first by round tag, not by basename (r04t sorted after r04ae)."""
    names = ["r05ab_traffic.json", "r05b_traffic.json", "r04ae_traffic.json", "r04t_traffic.json", "r06a_traffic.json",
             "r05z_c5_traffic.json"]
    got = [os.path.basename(p) for p in sorted(names, key=bench.profile_order)]
    assert got == ["r04t_traffic.json", "r04ae_traffic.json", "r05b_traffic.json", "r05z_c5_traffic.json",
                   "r05ab_traffic.json", "r06a_traffic.json"]


@pytest.mark.parametrize("steps,warmup,extra", [
    (20, 5, 2),   # the driver's run: warmup ends alone in slot 0, the timed run alone in slot 1
    (5, 2, 3),    # the default: warmup met beside-slot-0 only
    (20, 4, 0),   # warmup already met every graph of the timed run
    (4, 4, 0),
    (1, 1, 0),
    (2, 1, 2),
    (3, 0, 0),    # no warmup: nothing to complete
])
def test_warmup_completion(steps, warmup, extra):
    assert bench.warmup_completion(steps, warmup) == extra


def test_warmup_completion_covers_every_timed_graph():
    for steps in range(1, 12):
        for warmup in range(1, 8):
            extra = bench.warmup_completion(steps, warmup)
            have = bench.decode_graph_keys(warmup) | bench.decode_graph_keys(extra)
            assert bench.decode_graph_keys(steps) <= have, (steps, warmup, extra)
            assert extra <= 4


def test_plain_run_is_the_default_and_steps_are_checked(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "3"])
    a = bench.parse()
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 3)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "d"
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit):
        bench.parse()


def test_dump_outputs_writes_float_arrays(tmp_path):
    """--dump-outputs: ragged token lists become one -1 padded float32 matrix (token ids are exact in float32), with
    the counts and language ids beside it; a TurboTranscriber call adds its segment timestamps and text."""
    import numpy as np

    d = str(tmp_path / "out")
    bench.dump_outputs(d, [[50258, 50259, 51864], [7]], [50259, None],
                       {"text": "hé", "chunks": [{"timestamp": (0.0, 1.5), "text": "h"},
                                                 {"timestamp": (1.5, None), "text": "é"}]})
    got = {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}
    assert sorted(got) == ["languages", "text_codepoints", "timestamps", "token_counts", "tokens"]
    assert all(v.dtype in (np.float32, np.float64) for v in got.values())
    assert got["tokens"].tolist() == [[50258, 50259, 51864], [7, -1, -1]]
    assert got["token_counts"].tolist() == [3, 1] and got["languages"].tolist() == [50259, -1]
    assert got["timestamps"].shape == (2, 2) and np.isnan(got["timestamps"][1, 1]) and got["timestamps"][1, 0] == 1.5
    assert "".join(chr(int(c)) for c in got["text_codepoints"]) == "hé"
    bench.dump_outputs(d, [], [])  # nothing decoded: empty arrays, no error
    assert np.load(os.path.join(d, "tokens.npy")).shape == (0, 0)
