"""Every tools/*_rates.py runs end to end on a rehearsal world: a fresh child process per tool, 2 tiles of side 12 (288 bodies: the smallest world every
tool runs on, one size for all), a few thousand records, 2 blocks of 2 calls, the log in tmp_path.  The three tools that time a variant build beside
the tree's run in their --child mode, which measures the library the process loads and prints the JSON line alone (no log): no variant is built here.

A child that ends by a signal or at its time limit stops the module: the cases after it fail without starting another process on the GPU."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORLD = ["--tiles", "2", "--side", "12"]
LIMIT = 60           # seconds per child: every case measured 2.1 - 2.6 s on an MI355X box, most of it start-up; the rest is for a cold file cache
BLOCKS, REPEATS, INNER, N = ["--reps", "2"], ["--repeats", "2"], ["--inner", "2"], "4096"
# (in this one tool --side is the image's and comes after the world's --side, so it holds; the world's is --world-side)
SMALL_SENSORS = ["--world-side", "12", "--cameras", "16", "--side", "16", "--lidars", "4", "--rings", "8", "--azimuths", "64"]

# tool -> (arguments beside the world's, does its JSON line count records checked against the brute force)
CASES = {
    "query": (BLOCKS + ["--rays", N], False),
    "overlap": (BLOCKS + ["--queries", N], False),
    "spherecast": (BLOCKS + ["--casts", N], False),
    "boxcast": (BLOCKS + ["--casts", N], False),
    "capsulecast": (BLOCKS + ["--casts", N], False),
    "castall": (BLOCKS + REPEATS + ["--rays", N], False),
    "castk": (BLOCKS + REPEATS + ["--casts", N], True),
    "penetration": (BLOCKS + REPEATS + ["--queries", N], False),
    "closest": (BLOCKS + ["--queries", N, "--child"], False),
    "nearest": (BLOCKS + ["--queries", N, "--child"], False),
    "refit": (BLOCKS + ["--queries", N, "--child", "ab"], False),
    "distance": (BLOCKS + ["--queries", N], True),
    "filter": (BLOCKS + REPEATS + ["--queries", N], True),
    "move": (BLOCKS + REPEATS + ["--moves", N], True),
    "recover": (BLOCKS + REPEATS + ["--queries", N], True),
    "walk": (BLOCKS + REPEATS + ["--walks", N], True),
    "boxmove": (BLOCKS + REPEATS + ["--records", N], True),
    "touched": (BLOCKS + REPEATS + ["--records", N], True),
    "region": (BLOCKS + INNER + ["--cubes", "256"], False),
    "overlap_wide": (BLOCKS + INNER + ["--cubes", "256"], False),
    "events": (BLOCKS + INNER + ["--queries", N, "--cubes", "256"], False),
    "contact_events": (BLOCKS + INNER, False),
    "sense": (BLOCKS + INNER + SMALL_SENSORS, False),
}
FATAL = (124, 134, 137, 139)
_stopped = []          # why no further child is started


def profiles():
    d = os.path.join(ROOT, "profiles")
    return {f: (os.stat(os.path.join(d, f)).st_mtime_ns, os.stat(os.path.join(d, f)).st_size) for f in sorted(os.listdir(d))}


def checked_counts(node):
    """Every value under a key that counts records compared with the brute force, anywhere in the JSON tree."""
    if isinstance(node, dict):
        return [v for k, v in node.items() if k in ("checked", "checked_against_brute_force")] + [c for v in node.values() for c in checked_counts(v)]
    return [c for v in node for c in checked_counts(v)] if isinstance(node, list) else []


def test_every_rate_tool_has_a_case():
    tools = sorted(f[:-len("_rates.py")] for f in os.listdir(os.path.join(ROOT, "tools")) if f.endswith("_rates.py"))
    assert tools == sorted(CASES)


@pytest.mark.gpu
@pytest.mark.parametrize("tool", list(CASES))
def test_rate_tool_rehearsal(tool, tmp_path):
    assert not _stopped, f"not started: {_stopped[0]}"
    args, counts_checked = CASES[tool]
    out = tmp_path / f"{tool}_rates.log"
    env = {k: v for k, v in os.environ.items() if k != "NUDGE_HIP_LIBRARY"}
    before = profiles()
    try:
        child = subprocess.run([sys.executable, os.path.join(ROOT, "tools", f"{tool}_rates.py")] + WORLD + args + ["--out", str(out)],
                               env=env, capture_output=True, text=True, timeout=LIMIT, cwd=str(tmp_path))
    except subprocess.TimeoutExpired:
        _stopped.append(f"{tool}_rates.py was still running after {LIMIT} s")
        raise
    if child.returncode < 0 or child.returncode in FATAL:
        _stopped.append(f"{tool}_rates.py ended with status {child.returncode}")
    assert child.returncode == 0, f"status {child.returncode}\n{child.stdout[-2000:]}\n{child.stderr[-4000:]}"
    if "--child" in args:
        assert not out.exists()          # (the child protocol: the JSON line on stdout, the log is the parent's)
    else:
        assert out.read_text() == child.stdout
    last = json.loads(child.stdout.rstrip("\n").split("\n")[-1])
    assert isinstance(last, dict) and last
    if counts_checked:
        counts = checked_counts(last)
        assert counts and all(c > 0 for c in counts), f"a rehearsal that checks nothing: {counts}"
    assert profiles() == before
