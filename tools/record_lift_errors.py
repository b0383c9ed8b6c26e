#!/usr/bin/env python3
"""Record tests/golden/lift_errors_parent.json: (return code, p3d_last_error) of every bad call of
tests/lift_error_cases.py against ONE build of the library -- the build whose answers the next one
has to keep (tests/test_lift_errors.py).  No call reaches a launch, so this runs without a GPU.

    python tools/record_lift_errors.py PARENT/libp3d.so            # writes the fixture
    python tools/record_lift_errors.py PARENT/libp3d.so --check    # compares, writes nothing
    python tools/record_lift_errors.py PARENT/libp3d.so --gpu      # on a GPU: the rows behind a live filter and
                                                                   # behind a live model (tests/test_gpu_lift_errors.py) as well
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "3d-pose-baseline_amd"), os.path.join(ROOT, "tests")]
GOLD = os.path.join(ROOT, "tests", "golden", "lift_errors_parent.json")


def write(path, rows):
    with open(path, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r, sort_keys=True) for r in rows) + "\n]\n")
    print("%d rows -> %s" % (len(rows), os.path.relpath(path, ROOT)))


def main(argv):
    os.environ["P3D_LIB"] = os.path.abspath(argv[0])       # (everything in this process runs on that build)
    import _p3d
    import lift_error_cases
    rows = lift_error_cases.run(_p3d.lib())
    late = [r for r in rows if r["rc"] != _p3d.P3D_ERR_ARG]
    if late:
        raise SystemExit("not refused as a bad argument (it may have reached a launch): %r" % late[:3])
    if "--check" in argv:
        with open(GOLD) as f:
            want = json.load(f)
        bad = [(w, r) for w, r in zip(want, rows) if w != r]
        print("%d rows, %d differ" % (len(rows), len(bad) + abs(len(want) - len(rows))))
        for w, r in bad[:10]:
            print("  want %r\n  got  %r" % (w, r))
        return 1 if bad or len(want) != len(rows) else 0
    write(GOLD, rows)
    if "--gpu" in argv:
        import test_gpu_lift_errors
        rows = test_gpu_lift_errors.handle_rows()
        late = [r for r in rows if r["rc"] != _p3d.P3D_ERR_ARG]
        if late:
            raise SystemExit("not refused as a bad argument: %r" % late[:3])
        write(test_gpu_lift_errors.GOLD, rows)
        rows = test_gpu_lift_errors.lift_handle_rows()
        late = [r for r in rows if r["rc"] != _p3d.P3D_ERR_ARG]
        if late:
            raise SystemExit("not refused as a bad argument: %r" % late[:3])
        write(test_gpu_lift_errors.GOLD_LIFT, rows)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
