"""Writes tests/golden/launch_labels.json.gz: for every case of tests/test_launch_trace_host.py run with a recorder in
profiling.REC, the label and the algorithmic work (FLOP, bytes) of every bracketed launch, in order.  Data only; no GPU needed,
the library must be built.

    python tests/golden/make_golden_launch_labels.py            (writes the fixture)
    python tests/golden/make_golden_launch_labels.py --check    (records again and compares with the fixture on disk)

Run it under the rule of make_golden_launch_trace.py: only for a change that means to change what is launched or how it is
labelled, never for a refactoring of the host code.
"""
import gzip
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import test_launch_trace_host as T  # noqa: E402


def main(check):
    out = {}
    for case in T.CASES:
        out[case] = T.record(case, profiled=True)["brackets"]
        if out[case] != T.record(case, profiled=True)["brackets"]:
            raise SystemExit("not reproducible within one process: " + case)
        print(case, len(out[case]), "brackets")
    if check:
        with gzip.open(T.LABELS, "rt") as f:
            have = json.load(f)
        bad = [c for c in T.CASES if have.get(c) != out[c]]
        print("differ: " + ", ".join(bad) if bad else "identical to " + T.LABELS)
        raise SystemExit(1 if bad else 0)
    # one bracket per line, so that two decompressed versions diff launch by launch
    text = "{\n" + ",\n".join(json.dumps(c) + ": [\n" + ",\n".join(json.dumps(b, separators=(",", ":")) for b in out[c]) + "\n]"
                              for c in T.CASES) + "\n}\n"
    assert json.loads(text) == out
    with open(T.LABELS, "wb") as raw, gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0) as f:
        f.write(text.encode())
    print(T.LABELS, os.path.getsize(T.LABELS), "bytes")


if __name__ == "__main__":
    main("--check" in sys.argv[1:])
