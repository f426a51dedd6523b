"""Child process of tests/test_gpu_first_forward.py: ``python first_forward_child.py <scenario id>``.

The process does nothing on the GPU before its first patched forward.  It then runs three patch -> forward -> remove_patch
rounds of the scenario on fresh blocks under first_forward.record and prints one JSON line: the three digest lists, the
stages that held a non-finite float, and -- for the scenarios that have one -- the first round's error ratios against the
float64 restatement (first_forward.reference_ratios).  Any failure is an exception, so the process ends at once with a
non-zero status and starts nothing further; a watchdog ends it if it hangs."""
import faulthandler
import json
import os
import sys

TESTS = os.path.dirname(os.path.abspath(__file__))
for p in (TESTS, os.path.dirname(TESTS)):
    if p not in sys.path:
        sys.path.insert(0, p)

LIMIT_S = 150            # a round takes a second or two; the float64 restatement on the host a few more
REFERENCED = ("s9", "odd")


def main(name):
    faulthandler.dump_traceback_later(LIMIT_S, exit=True)
    import torch

    import first_forward as FF
    assert not torch.cuda.is_initialized(), "the GPU was touched before the first patched forward"
    runs, nonfinite, first = [], [], None
    for i in range(3):
        rec = FF.run_scenario(name, "cuda", keep=FF.KEEP if (i == 0 and name in REFERENCED) else ())
        torch.cuda.synchronize()
        first = rec if first is None else first
        runs.append([list(e) for e in rec])
        nonfinite.append(rec.nonfinite)
    ratios = FF.reference_ratios(name, first) if name in REFERENCED else None
    faulthandler.cancel_dump_traceback_later()
    print("FIRST_FORWARD " + json.dumps({"scenario": name, "runs": runs, "nonfinite": nonfinite, "ratios": ratios}))


if __name__ == "__main__":
    main(sys.argv[1])
