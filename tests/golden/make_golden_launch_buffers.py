"""Writes tests/golden/launch_buffers.json.gz: for every case of tests/test_launch_trace_host.py and every launch of its trace, the
plan-held buffer (``"a<k>+<byte offset>"``) or ``"p"`` behind each pointer that launch_trace.json.gz records as ``"p"``, as that
test's docstring describes them.  Data only; no GPU needed, the library must be built.

    python tests/golden/make_golden_launch_buffers.py            (writes the fixture)
    python tests/golden/make_golden_launch_buffers.py --check    (records again and compares with the fixture on disk)

Run it under the rule of make_golden_launch_trace.py: only for a change that means to change what is launched or which buffer a
launch takes, never for a refactoring of the host code.  Each case is recorded twice and the script aborts if the two records
differ; before a new fixture is committed, ``--check`` from a second, fresh process must find it identical.
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
        out[case] = T.record(case, buffers=True)["buffers"]
        again = T.compare_buffers(case, out[case], T.record(case, buffers=True))
        if again is not None:
            raise SystemExit("not reproducible within one process: " + again)
        names = [e for row in out[case] for e in row]
        print(case, len(out[case]), "launches,", sum(e != "p" for e in names), "pointers named,", names.count("p"), "left")
    if check:
        with gzip.open(T.BUFFERS, "rt") as f:
            have = json.load(f)
        bad = [c for c in T.CASES if have.get(c) != out[c]]
        print("differ: " + ", ".join(bad) if bad else "identical to " + T.BUFFERS)
        raise SystemExit(1 if bad else 0)
    # one launch per line, as launch_trace.json.gz has them
    text = "{\n" + ",\n".join(json.dumps(c) + ": [\n" + ",\n".join(json.dumps(row, separators=(",", ":")) for row in out[c]) + "\n]"
                              for c in T.CASES) + "\n}\n"
    assert json.loads(text) == out
    with open(T.BUFFERS, "wb") as raw, gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0) as f:
        f.write(text.encode())
    print(T.BUFFERS, os.path.getsize(T.BUFFERS), "bytes")


if __name__ == "__main__":
    main("--check" in sys.argv[1:])
