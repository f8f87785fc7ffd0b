#!/usr/bin/env python
"""Same-box A/B of library builds at other batch sizes than the bench's (tools/ab_headline.py is the headline's): alternates the
builds (MKH_LIB_TAG values, '' = product) in separate processes and prints the kernel ms (mean, median) of each round.
    python tools/ab_batch.py "" parent --batches 4096,8192,10240 [--rounds 5] [--config g1_c3]
Stops at the first process that does not end cleanly."""
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTS = ("--config", "--rounds", "--batches")
tags = [a for i, a in enumerate(sys.argv[1:], 1) if not a.startswith("--") and sys.argv[i - 1] not in OPTS]
opt = lambda name, default: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default
cfg, rounds = opt("--config", "g1_c3"), int(opt("--rounds", "5"))
batches = [int(b) for b in opt("--batches", "4096,8192,10240").split(",")]
code = ("import sys; sys.path.insert(0, %r); import bench, torch; "
        "o = bench.measure_side_config(%r, torch.device('cuda', 0), steps=40, warmup=5, batch=int(sys.argv[1])); "
        "print('%%s %%.4f %%.4f' %% (o['kernel'], o['kernel_ms'], o['kernel_ms_median']))") % (REPO, cfg)
for B in batches:
    res = {t: [] for t in tags}
    for r in range(rounds):
        for t in tags:
            p = subprocess.run([sys.executable, "-c", code, str(B)], env=dict(os.environ, MKH_LIB_TAG=t), capture_output=True, text=True, timeout=300)
            if p.returncode != 0:
                sys.exit("batch %d, build %r: exit status %d\n%s" % (B, t, p.returncode, p.stderr[-500:]))
            res[t].append(p.stdout.strip().split("\n")[-1])
    for t in tags:
        print(B, "[%s]" % (t or "product"), " | ".join(res[t]), flush=True)
