"""Host-side AddressSanitizer run of the C-ABI (SURVEY.md §5 "Race detection /
sanitizers": `-fsanitize=address` host builds of the C-ABI). GPU ASan is not available on
this pool, so every libisg source is rebuilt with the host half instrumented
(tools/asan/build.sh, -Xarch_host -fsanitize=address) and linked into
tools/asan/abi_host_check.cpp, which drives the argument validation, error plumbing,
executor record parsing / pointer fix-ups and host item-array chunking with valid and
malformed inputs. Any ASan report fails the test. No GPU is needed (launches fail
cleanly without a device).

The executor's stream order (csrc/exec.cpp) has a host program of its own,
tools/asan/exec_order_check.cpp: the executor against recording stubs, under ASan + UBSan,
on synthetic op lists and on a plan's real ones."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_host_paths_under_asan():
    out = os.path.join(ROOT, "tools", "asan", "_build")
    b = subprocess.run(["bash", os.path.join(ROOT, "tools", "asan", "build.sh"), out],
                       capture_output=True, text=True, timeout=1200)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:exitcode=23")
    r = subprocess.run([os.path.join(out, "abi_host_check")], capture_output=True, text=True,
                       timeout=300, env=env)
    print(r.stdout)
    assert "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert "OK: 0 failure(s)" in r.stdout


def test_executor_stream_order_matches_the_python_mirror(tmp_path):
    """exec_order_check on the op lists of a real plan: the ordering properties hold, and for
    every main-stream record the side records the executor has made the main stream wait for
    include every one tests/test_host_cpu.py::_joined_before lists — the Python mirror of
    "the executor's rule", which the planner's fork/join tests are checked against. (The
    executor's set may be larger: a join closes whole batches, the mirror knows of none.)"""
    from instancesegmentation_amd.engine import Plan, Record
    from instancesegmentation_amd.model.segment import Segment
    from tests.test_host_cpu import _joined_before

    out = os.path.join(ROOT, "tools", "asan", "_build")
    b = subprocess.run(["bash", os.path.join(ROOT, "tools", "asan", "build.sh"), out, "order"],
                       capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    exe = os.path.join(out, "exec_order_check")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:exitcode=23",
               UBSAN_OPTIONS="halt_on_error=1:exitcode=24")

    def run(args):
        r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300, env=env)
        assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
        assert r.returncode == 0, (args, r.returncode, r.stdout[-2000:], r.stderr[-2000:])
        assert "OK: 0 failure(s)" in r.stdout
        return r.stdout

    run([])  # the synthetic lists and the error cases

    p = Plan(Segment(20), [(2, 3, 128, 128), (2, 17, 3)], True, True, (False, False))
    side_idx = [i for i, r in enumerate(p.fwd.recs) if r.flags & Record.OPF_SIDE]
    lists = [("fwd", p.fwd, ["--side"]), ("bwd", p.bwd, ["--side"]), ("bwd2", p.bwd, ["--side2"])]
    lists += [(f"stamped{idx}", p.fwd.stamped(idx), ["--side"]) for idx in side_idx[:3] + side_idx[-3:]]
    compared = 0
    for name, ol, mode in lists:
        path = tmp_path / f"{name}.blob"
        path.write_bytes(ol.blob)
        text = run(["--blob", str(path), "--nops", str(len(ol.recs))] + mode)
        got = {int(m.group(1)): {int(t) for t in m.group(2).split()}
               for m in re.finditer(r"^main (\d+):([ \d]*)$", text, re.M)}
        mains = [k for k, r in enumerate(ol.recs) if not r.flags & Record.OPF_SIDE]
        assert sorted(got) == mains, name
        for k in mains:
            want = _joined_before(ol.recs, k)
            assert want <= got[k], (name, k, ol.recs[k].label, sorted(want - got[k]))
            compared += len(want)
    assert compared > 100  # the mirror had something to say
