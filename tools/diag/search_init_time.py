"""Single-call latency of guided-search mode 1 (SearchForInitialization, host pointers): windows of 100 pixels, where the stored
candidate lists serve every re-scan, and windows over the whole frame, where a stale query walks the frame's keypoints again."""
import sys, time
sys.path.insert(0, ".")
from weiner_slamit_v2_amd import api, synth  # noqa: E402

for name, (n, seed, window) in (("1500 keypoints, window 100", (1500, 0, 100)), ("1600 keypoints, window 2000 (lists truncated)", (1600, 5, 2000))):
    f1, prev, f2 = synth.synth_init_pair(n, seed)
    api.ORBmatcher.search_for_initialization(f1, prev, f2, window, 0.9, 50)
    r = []
    for _ in range(50):
        t0 = time.perf_counter(); g = api.ORBmatcher.search_for_initialization(f1, prev, f2, window, 0.9, 50); r.append(time.perf_counter() - t0)
    r.sort()
    print("%-50s HIP median %.3f ms  (%d matches)" % (name, 1e3 * r[25], g[1]))
