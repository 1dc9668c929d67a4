"""Scenarios of tests/fresh_scenarios.py in a FRESH child process (test helper, not a conftest).

Two kinds of behaviour are fixed once per process, so the one pytest process of the suite cannot see them: kernels selected by an
environment variable that the library reads once into a `static`, and kernels whose first launch of the process happens inside a graph
capture (engine.hip: warm_kernels).  `run` starts one child per call with `subprocess.run` — never an exec of this process —, children
run one at a time, each with its own timeout.  The child imports `__graft_entry__`, calls `load_package()`, looks the scenario up by
name, calls it as `f(pkg, *args)` and prints one line `FRESH_RESULT <json>`; whatever else it prints (the `WORST` lines) is passed on.

Once a child has ended by a signal or at its timeout, every later `run` of this process fails at once without starting a child:
nothing more is started on a GPU that may have faulted, and nothing is retried."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAG = "FRESH_RESULT "
FATAL_CODES = (124, 134, 137, 139)

dead = None   # why no further child is started (set once)

_CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import __graft_entry__ as graft
import fresh_scenarios
pkg = graft.load_package()
out = getattr(fresh_scenarios, sys.argv[2])(pkg, *json.loads(sys.argv[3]))
sys.stdout.flush()
print(sys.argv[4] + json.dumps(out), flush=True)
"""


def run(scenario_name, env=None, timeout=300, args=()):
    """The scenario's result from a fresh child whose environment is os.environ with `env` merged over it."""
    global dead
    assert dead is None, "no child started: " + dead
    what = "%s%s %s" % (scenario_name, tuple(args), env or {})
    try:
        res = subprocess.run([sys.executable, "-c", _CHILD, ROOT, scenario_name, json.dumps(list(args)), TAG], capture_output=True, text=True,
                             timeout=timeout, env=dict(os.environ, **(env or {})))
    except subprocess.TimeoutExpired:
        dead = "%s did not end within %d s" % (what, timeout)
        raise AssertionError(dead)
    lines = res.stdout.splitlines()
    for line in lines:
        if not line.startswith(TAG):
            print(line)
    if res.returncode < 0 or res.returncode in FATAL_CODES:
        dead = "%s ended with return code %d" % (what, res.returncode)
        raise AssertionError(dead + "\n" + res.stderr[-2000:])
    assert res.returncode == 0, "%s failed (return code %d)\n%s" % (what, res.returncode, res.stderr[-4000:])
    got = [line for line in lines if line.startswith(TAG)]
    assert len(got) == 1, "%s printed %d result lines" % (what, len(got))
    return json.loads(got[0][len(TAG):])
