"""Writes tests/golden/launch_trace.json.gz: for every case of tests/test_launch_trace_host.py, the calls the engines and fused
trainers make into the HIP library in dry-run mode (no GPU needed; the library must be built).  Data only: names and argument
values, as that test's docstring describes them.

    python tests/golden/make_golden_launch_trace.py            (writes the fixture)
    python tests/golden/make_golden_launch_trace.py --check    (records again and compares with the fixture on disk)

Run it only for a change that means to change what is launched, and review the difference it makes to the fixture.  Each case
is recorded twice and the script aborts if the two records differ: whatever the trace holds must not depend on the process's
memory layout.
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
        out[case] = T.record(case)
        again = T.compare(case, out[case], T.record(case))
        if again is not None:
            raise SystemExit("not reproducible within one process: " + again)
        print(case, len(out[case]["launches"]), "launches,", len(out[case]["queries"]), "queries")
    if check:
        with gzip.open(T.FIXTURE, "rt") as f:
            have = json.load(f)
        bad = [m for m in (T.compare(c, have[c], out[c]) for c in T.CASES) if m]
        print("\n".join(bad) if bad else "identical to " + T.FIXTURE)
        raise SystemExit(1 if bad else 0)
    # one call per line, so that two decompressed versions diff call by call
    text = "{\n" + ",\n".join(
        json.dumps(c) + ": {" + ", ".join(
            json.dumps(part) + ": [\n" + ",\n".join(json.dumps(x, sort_keys=True, separators=(",", ":")) for x in out[c][part]) + "\n]"
            for part in ("launches", "queries", "tables")) + "}"
        for c in T.CASES) + "\n}\n"
    assert json.loads(text) == out
    with open(T.FIXTURE, "wb") as raw, gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0) as f:
        f.write(text.encode())
    print(T.FIXTURE, os.path.getsize(T.FIXTURE), "bytes")


if __name__ == "__main__":
    main("--check" in sys.argv[1:])
