"""The launch trace of the field backward executor (csrc/field_bwd.cpp), pinned on the CPU.

The executor is host code only: it calls nerf_* entries, a few nerf:: internals and three HIP event
functions.  tests/native/field_bwd_trace.cpp replaces all of them by stubs that print their arguments
(pointers symbolically) and drives both entries through every schedule knob, every refusal and every
mid-schedule failure in one process.  The program is linked without the HIP runtime, so a HIP call
left in the executor is a link error.  Its output must equal the trace recorded from the executor as
it was before its pieces were shared: tests/golden/field_bwd_trace.sha256 holds one line per case
(name, lines, sha256), tests/golden/field_bwd_trace_default.txt the full text of the four default
cases.  A changed launch, argument, stream, event, message or return code changes a digest.

Re-record the golden files only for a deliberate change of the schedule, from a source whose trace
was reviewed (a plain run of this file records nothing):
    python tests/test_field_bwd_trace.py --record
"""
import difflib
import hashlib
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "my-nope-nerf_amd", "csrc", "field_bwd.cpp")
HARNESS = os.path.join(ROOT, "tests", "native", "field_bwd_trace.cpp")
DIGESTS = os.path.join(ROOT, "tests", "golden", "field_bwd_trace.sha256")
SPECIMEN = os.path.join(ROOT, "tests", "golden", "field_bwd_trace_default.txt")
FULL_TEXT = ("chain/s64/unset/rg0", "chain/s64/unset/rg1", "rays/graw4", "rays/composite")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def build_and_run(out_dir):
    """The harness built host-only (no device pass, no HIP runtime) into out_dir; its stdout."""
    exe = os.path.join(str(out_dir), "field_bwd_trace")
    cmd = [HIPCC, "-x", "hip", "--offload-host-only", "-no-hip-rt", "-std=c++17", "-O1", "-Wall", CSRC, HARNESS,
           "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, f"{' '.join(cmd)}\n{r.stdout}\n{r.stderr}"
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, f"the harness ended with {r.returncode}\n{r.stderr[-2000:]}"
    return r.stdout


def split_cases(text):
    """{case: [lines]} in order of appearance ('== <case>' opens one)."""
    cases, cur = {}, None
    for line in text.splitlines():
        if line.startswith("== "):
            name = line[3:]
            assert name not in cases, f"case {name} appears twice"
            cur = cases[name] = []
        else:
            assert cur is not None, "trace line before the first case"
            cur.append(line)
    return cases


def digest(lines):
    return hashlib.sha256("".join(l + "\n" for l in lines).encode()).hexdigest()


def specimen_text(cases):
    return "".join(f"== {n}\n" + "".join(l + "\n" for l in cases[n]) for n in FULL_TEXT)


@pytest.fixture(scope="module")
def trace(tmp_path_factory):
    """(cases, path of the full actual trace): the harness built and run once for the module."""
    out = tmp_path_factory.mktemp("field_bwd_trace")
    text = build_and_run(out)
    actual_path = out / "field_bwd_trace_actual.txt"
    actual_path.write_text(text)      # kept for a look after a mismatch
    return split_cases(text), actual_path


def test_trace_equals_the_recorded_one(trace):
    cases, actual_path = trace
    with open(DIGESTS) as f:
        golden = [l.split() for l in f.read().splitlines() if l and not l.startswith("#")]
    assert [g[0] for g in golden] == list(cases), (
        f"the list of cases differs from {DIGESTS}: "
        f"missing {sorted(set(g[0] for g in golden) - set(cases))}, new {sorted(set(cases) - set(g[0] for g in golden))}, "
        f"or another order; full trace in {actual_path}")
    with open(SPECIMEN) as f:
        want = split_cases(f.read())
    assert tuple(want) == FULL_TEXT
    for name in FULL_TEXT:      # first: these fail with a readable diff
        if cases[name] != want[name]:
            diff = "\n".join(difflib.unified_diff(want[name], cases[name], "recorded", "actual", lineterm="", n=1))
            raise AssertionError(f"case {name}: the trace changed (full trace in {actual_path})\n{diff}")
    bad = [name for name, n_lines, sha in golden
           if (len(cases[name]), digest(cases[name])) != (int(n_lines), sha)]
    assert not bad, f"{len(bad)} case(s) changed, the first: {bad[0]} (all: {bad}); full trace in {actual_path}"


def test_refusals_precede_every_launch(trace):
    """What the digests pin, readably: a refused call has set a message and launched nothing; a failed
    launch after the side stream was forked ends with the join (record on side, wait on main)."""
    cases = trace[0]
    refused = [n for n in cases if n.startswith("refuse/") and "/ok/" not in n]
    assert len(refused) > 60
    for n in refused:
        assert cases[n][-1] == "return rc=-1 launches=0", (n, cases[n][-1])
        assert sum(l.startswith("set_error ") for l in cases[n]) == 1, n
    failed = [n for n in cases if n.startswith("fail/") and cases[n][-1].startswith("return rc=-2")]
    assert len(failed) > 100
    for n in [n for n in failed if not n.startswith("fail/rays/")]:
        assert cases[n][-3].startswith("hipEventRecord side ev") and cases[n][-2].startswith("hipStreamWaitEvent main ev"), n


if __name__ == "__main__":
    import tempfile
    if sys.argv[1:] != ["--record"]:
        sys.exit("nothing recorded: pass --record to overwrite the golden trace with this source's")
    with tempfile.TemporaryDirectory() as d:
        cs = split_cases(build_and_run(d))
    with open(DIGESTS, "w") as f:
        f.write("# case, trace lines, sha256 of them (tests/test_field_bwd_trace.py)\n")
        f.writelines(f"{n} {len(ls)} {digest(ls)}\n" for n, ls in cs.items())
    with open(SPECIMEN, "w") as f:
        f.write(specimen_text(cs))
    print(f"{len(cs)} cases -> {DIGESTS}, {SPECIMEN}", file=sys.stderr)
