"""bench.py on a small drop scene (pytest -m gpu): `--steps K` is the number of timed steps, and `--dump-outputs` writes what the last timed step computed --
the same arrays, bit for bit, from two runs with the same arguments (seeded inputs, deterministic step), so that two builds can be compared output for output."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
SMALL = ["--tiles", "2", "--side", "30", "--warmup", "2", "--no-cpu", "--no-full-window"]


def _run(cmd, env=None):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


@pytest.mark.gpu
def test_steps_is_the_number_of_timed_steps_and_dumps_repeat_bit_for_bit(tmp_path):
    outs, dumps = [], []
    for run in ("a", "b"):
        outs.append(_run([sys.executable, BENCH, "--gpus", "1", "--steps", "7"] + SMALL + ["--dump-outputs", str(tmp_path / run)]))
        dumps.append(_load(str(tmp_path / run)))
    for out in outs:
        assert out["steps"] == 7 and out["config"]["timed_steps"] == 7 and out["config"]["timed_blocks"] == 1, out["config"]
    a, b = dumps
    assert sorted(a) == sorted(b)
    for name in a:
        assert a[name].dtype in (np.float32, np.float64), name
        assert a[name].dtype == b[name].dtype and a[name].shape == b[name].shape and a[name].tobytes() == b[name].tobytes(), name
    nb = 2 * 30 * 30 + 1                                                 # (+ the static body 0)
    assert np.array_equal(a["body_index"], np.arange(nb, dtype=np.float64))
    contacts, _, active, cache = a["counts"]
    assert contacts > 0.9 * 4 * (nb - 1) and active >= nb - 1 and cache > 0
    assert len(a["contact_position"]) == contacts and len(a["cache_impulse"]) == cache
    assert np.all(np.isfinite(a["body_position"])) and np.all(a["body_position"][1:, 1] > -10.0)      # landed on the slabs, not through them


@pytest.mark.gpu
def test_partitioned_bench_dumps_the_gathered_world():
    """The partitioned path (one rank over RCCL loopback, as in test_gpu_partition.py): rank 0 dumps the owned bodies of all ranks, merged by global id."""
    import tempfile
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    with tempfile.TemporaryDirectory() as d:
        env = dict(os.environ, NUDGE_BENCH_LOOPBACK="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
        out = _run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1", "--master-port", str(port),
                    BENCH, "--gpus", "1", "--steps", "5"] + SMALL + ["--dump-outputs", d], env=env)
        assert out["config"]["timed_steps"] == 5
        a = _load(d)
    assert np.array_equal(a["body_index"], np.arange(1, 2 * 30 * 30 + 1, dtype=np.float64))
    assert np.all(np.isfinite(a["body_position"])) and np.all(a["body_position"][:, 1] > -10.0)
