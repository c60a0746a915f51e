"""One EM call (50 steps) at the headline or the stress shape, for a rocprofv3 --kernel-trace --stats run:
    rocprofv3 --kernel-trace --stats -d profiles/em/rocprof -o em -- python tools/em_prof_case.py headline stress"""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))

import em_speed                                   # noqa: E402
from sbayes_amd import em                        # noqa: E402

for name in sys.argv[1:] or ["headline", "stress"]:
    x, app, avail, k, z0 = em_speed.golden_case(name) if name != "stress" else em_speed.workload_case(name)
    h = em.EmHandle(x, app, avail, k, device=0)
    h.run(z0, em.temperatures(50))
    print(name, "kernel ms", h.last_kernel_ms(), flush=True)
    h.close()
