"""Writes tests/golden/assign_schedule.json: what the two ``run`` loops of the assignment phase (``run_robot.AssignmentPhase.run``
and ``run_robot.AssignmentPhaseBatch.run``) do, call for call, over a grid of schedules.  tests/test_assign_phase_cpu.py holds
the one ``run`` that replaced them to these sequences.

The file is a record of ONE commit, the last one with two ``run`` methods: it MUST be generated in a checkout of that commit
(the parent of the change that merged the two classes), never from the tree under test.  There the methods are called unbound on
a stub object that has what they read -- ``gap``, ``_have``, ``capture_guard``, ``refresh()`` and the stepper under its old
names ``eng`` / ``batch``.  Usage:

    python tests/golden/make_golden_assign_schedule.py <commit id>

No GPU is needed: the loops are host logic.

A sequence is a string of words: ``r`` a refresh, ``c<k>`` capture(steps_per_graph=k) (it runs one iteration), ``s<k>`` step(k),
``n<i>`` on_snapshot(i).  A case is [assign_gap, first iteration, iterations, snapshot_gap, first]: ``first`` is what the first
refresh returns (True: the engine's mode changed; every later refresh returns False); the solo form runs with a snapshot
callback at snapshot_gap 0 (a snapshot at the end only) and 3.  The batch form has no snapshots: its sequences are recorded
on their own and are the solo ones without the ``n`` words, which this script asserts."""
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "assign_schedule.json")

GAPS, STARTS, ITERS, SNAPSHOT_GAPS, FIRST = (1, 2, 5), range(7), range(13), (0, 3), (True, False)


class Stub:
    """Stands for ``self`` of a ``run``, and for the stepper behind it."""

    def __init__(self, gap, first):
        self.gap, self._have, self.capture_guard, self.log = gap, False, None, []
        self.eng = self.batch = self
        self._first = first

    def refresh(self):
        self.log.append("r")
        first, self._first, self._have = self._first, False, True
        return first

    def capture(self, steps_per_graph=1):
        self.log.append(f"c{steps_per_graph}")
        return 1

    def step(self, n=1):
        self.log.append(f"s{n}")

    def snapshot(self, i):
        self.log.append(f"n{i}")


def collect():
    sys.path.insert(0, ROOT)
    from reart_amd import run_robot as rr

    solo, batch = [], []
    for gap, start, iters, first in itertools.product(GAPS, STARTS, ITERS, FIRST):
        plain = None
        for sg in SNAPSHOT_GAPS:
            s = Stub(gap, first)
            assert rr.AssignmentPhase.run(s, start, start + iters, sg, s.snapshot) == start + iters
            solo.append([[gap, start, iters, sg, first], " ".join(s.log)])
            if sg == 0:
                plain = [w for w in s.log if not w.startswith("n")]
        s = Stub(gap, first)
        assert rr.AssignmentPhase.run(s, start, start + iters) == start + iters and s.log == plain     # no callback: nothing else moves
        s = Stub(gap, first)
        assert rr.AssignmentPhaseBatch.run(s, start, start + iters) == start + iters
        assert s.log == plain, (gap, start, iters, first, s.log, plain)
        batch.append([[gap, start, iters, 0, first], " ".join(s.log)])
    return solo, batch


if __name__ == "__main__":
    commit = sys.argv[1]
    solo, batch = collect()
    with open(OUT, "w") as f:
        f.write('{"commit":' + json.dumps(commit) + ',\n')
        for name, rows, end in (("solo", solo, ","), ("batch", batch, "")):
            f.write(json.dumps(name) + ":[\n" + ",\n".join(json.dumps(r, separators=(",", ":")) for r in rows) + "\n]" + end + "\n")
        f.write("}\n")
    print(OUT, len(solo), "solo and", len(batch), "batch sequences")
