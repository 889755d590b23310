"""Launch sequence of the IPC-window schedule walker, pinned without a GPU.

csrc/tests/p2p_issue_trace.cpp walks the real schedules and plans through
P2pGroup::IssueSchedule on a hand-built group with recording launchers, under
ASan/UBSan, and prints one digest line per case and rank. The golden lines
were recorded before the walker was split into stages: any change to what it
launches, in which order or with which argument shows up here as a diff.
`build/p2p_issue_trace_asan --dump CASE` prints a case's launches in full.
"""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "p2p_issue_trace.txt")


def test_p2p_issue_trace_matches_golden():
    exe = os.path.join(REPO, "build", "p2p_issue_trace_asan")
    subprocess.run(["make", "p2p-trace"], cwd=REPO, check=True,
                   capture_output=True, timeout=900)
    got = []
    # the walker reads MLSL_P2P_FUSED_MAX_KB once per process
    for fused_max_kb in (None, "0"):
        env = {k: v for k, v in os.environ.items() if k != "MLSL_P2P_FUSED_MAX_KB"}
        env["UBSAN_OPTIONS"] = "halt_on_error=1"   # UBSan only prints by default
        if fused_max_kb is not None:
            env["MLSL_P2P_FUSED_MAX_KB"] = fused_max_kb
        out = subprocess.run([exe], env=env, capture_output=True, text=True,
                             timeout=300)
        # a sanitizer report makes the exit status non-zero
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
        got += out.stdout.splitlines()
    with open(GOLDEN) as f:
        want = f.read().splitlines()
    assert len(got) == len(want), (len(got), len(want))
    for g, w in zip(got, want):
        assert g == w, f"got {g!r}, golden {w!r}"
