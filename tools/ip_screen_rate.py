"""How often the fp64 blocks behind ImageProjection's f32 screens (csrc/ip_pred.h) are entered: wavefront passes of ip_fused_t's phase B, or wavefronts
of ipb_band, that held at least one undecided ground pair / edge site, over the synthetic streams bench.py replays.  Needs a library built with
-DALEGO_TIMING (a-lego-loam_amd/build.sh).
usage: ALEGO_LIB=a-lego-loam_amd/libalego_timing.so python tools/ip_screen_rate.py [geometry=16x1800] [streams=64] [scans=40]"""
import ctypes as C, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from alego_loader import load_package; load_package()
from alego_amd import binding, synth
ns, hs = (int(v) for v in (sys.argv[1] if len(sys.argv) > 1 else "16x1800").split("x"))
B = int(sys.argv[2]) if len(sys.argv) > 2 else 64
K = int(sys.argv[3]) if len(sys.argv) > 3 else 40
p = synth.default_params(ns, hs)
h = binding.Handle(p, n_slots=B, ring_len=K)
for s in range(B):
    for k in range(K):
        h.batch_load(s, k, synth.scan(p, k, stream=s))
fn = binding.lib().alego_iph_slow_counts if ns <= 16 else binding.lib().alego_ipb_slow_counts
t = (C.c_ulonglong * 4)()
fn(t, 1)
h.batch_run(0, K, 1)
fn(t, 0)
allp, g, e = int(t[0]), int(t[1]), int(t[2])
print(f"{ns}x{hs}, {B} streams x {K} scans: {allp} wavefront passes; fp64 block entered for ground pairs {g} ({100.0 * g / max(allp, 1):.4f} %), for edge sites {e} ({100.0 * e / max(allp, 1):.4f} %)")
h.close()
