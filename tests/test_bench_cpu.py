"""bench.py's self-launch: `python bench.py --gpus N` with no
WORLD_SIZE in the environment starts N rank processes of itself (the env
torch.distributed.run would set) before anything touches a GPU, and passes
rank 0's one JSON line through.  Checked with the launcher rehearsal
(--launch-check: gloo rendezvous + all-reduce, no GPU)."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_spawns_its_ranks():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "3", "--launch-check"],
                       env=env, capture_output=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    # (gloo itself prints a "[Gloo] Rank 0 is connected" line on stdout)
    lines = [l for l in r.stdout.decode().splitlines() if l.startswith("{")]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    assert d["n_gpus"] == 3 and d["rank_sum"] == 3.0


def test_dump_outputs_files(tmp_path):
    """--dump-outputs: one float32 (float64 kept) .npy per output; an output
    above DUMP_SAMPLE elements is a sample at indices fixed by its size, so
    two dumps of the same values are equal file for file."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    n = bench.DUMP_SAMPLE + 12344
    big = torch.arange(n, dtype=torch.float32).reshape(2, -1)
    outs = {"big": big, "small": torch.arange(6, dtype=torch.int32).reshape(2, 3),
            "half": torch.tensor([0.5, 1.5], dtype=torch.float16), "wide": torch.tensor([1.0 / 3], dtype=torch.float64)}
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    bench.dump_outputs(a, outs)
    bench.dump_outputs(b, {k: v.clone() for k, v in outs.items()})
    assert sorted(os.listdir(a)) == ["big.npy", "half.npy", "small.npy", "wide.npy"]
    total = 0
    for f in os.listdir(a):
        x, y = np.load(os.path.join(a, f)), np.load(os.path.join(b, f))
        assert x.dtype == (np.float64 if f == "wide.npy" else np.float32) and np.array_equal(x, y)
        total += x.nbytes
    assert total <= bench.DUMP_MAX_BYTES
    s = np.load(os.path.join(a, "big.npy"))
    # the sample holds elements of the output itself (arange: value = flat index), spread over all of it
    assert s.shape == (bench.DUMP_SAMPLE,) and np.all(np.diff(s) >= 0) and s[0] < n // 100 and s[-1] > n - n // 100
    assert np.array_equal(np.load(os.path.join(a, "small.npy")), np.arange(6, dtype=np.float32))
    assert np.load(os.path.join(a, "wide.npy"))[0] == 1.0 / 3
