"""bench.py command line: the result line and --dump-outputs on the tiny
config. The runs happen in one child process with the GPUs hidden, so
they neither need a device nor switch TunableOp on inside the test
process."""

import json
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import bench  # noqa: E402

TINY = ["--gpus", "1", "--model", "tiny", "--batch-per-gpu", "4",
        "--prompt-len", "16", "--new-tokens", "6"]

CHILD = """
import json, sys
import bench
for argv in json.loads(sys.argv[1]):
    sys.argv = ["bench.py"] + argv
    bench.main()
"""


def test_dump_outputs_reproducible(tmp_path):
    """Two runs with the same model and prompts dump identical float64
    arrays of what generate() returned; --steps sets the timed steps;
    --full and another step count do not change what a step computes."""
    runs = [TINY + ["--steps", "2", "--warmup", "1",
                    "--dump-outputs", str(tmp_path / "a")],
            TINY + ["--steps", "1", "--warmup", "0", "--full",
                    "--dump-outputs", str(tmp_path / "b")]]
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    out = subprocess.run([sys.executable, "-c", CHILD, json.dumps(runs)],
                         cwd=REPO, env=env, capture_output=True, text=True,
                         timeout=240)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.strip().splitlines()
    assert len(lines) == 2, lines          # one result line per run
    a, b = (json.loads(ln) for ln in lines)
    assert a["steps"] == 2 and b["steps"] == 1
    for r in (a, b):
        assert r["ms_per_step"] > 0 and r["unit"] == "tokens/s"
        assert r["higher_is_better"] is True
        assert r["dtype"] in ("fp32", "bf16")
        # value and ms_per_step describe the same timed window
        tokens = r["config"]["global_batch"] * r["config"]["new_tokens"]
        assert abs(r["value"] * r["ms_per_step"] / 1e3 - tokens) \
            < 1e-6 * tokens
    assert os.listdir(tmp_path / "a") == ["tokens.npy"]
    ta = np.load(tmp_path / "a" / "tokens.npy")
    tb = np.load(tmp_path / "b" / "tokens.npy")
    assert ta.dtype == np.float64 and ta.shape == (4, 6)
    assert np.array_equal(ta, tb)
    assert np.all(ta == np.round(ta)) and ta.min() >= 0


def test_dump_outputs_size_cap(monkeypatch, tmp_path):
    """An output over the byte budget is cut to a fixed seeded sample."""
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 8 * 100)
    big = np.arange(1000, dtype=np.float32)
    for d in ("x", "y"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "small": [1.5]})
    x = np.load(tmp_path / "x" / "big.npy")
    assert x.dtype == np.float64 and x.shape == (50,)
    assert np.array_equal(x, np.load(tmp_path / "y" / "big.npy"))
    assert np.all(np.diff(x) > 0) and set(x) <= set(big.tolist())
    assert np.load(tmp_path / "x" / "small.npy").tolist() == [1.5]
