#!/usr/bin/env python3
"""Shader-clock stamps inside base_fwd_kernel / base_bwd_block_kernel (workgroup 1; thread 0, and lane 0 of one wave per role).
    make -C reart_amd/csrc stats && REART_LIB=reart_amd/csrc/libreart_hip_stats.so python tools/phase_clock.py"""
import ctypes, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch, bench
from reart_amd import _lib
eng, seq, model = bench.build_instance(torch.device("cuda:0"), 20, 4096, 0, 2)
lib = ctypes.CDLL(_lib.LIB_PATH)
buf = (ctypes.c_ulonglong * 32)()
pbuf = (ctypes.c_ulonglong * 8)()
TICK_US = 1e-2        # replaced below by the measured rate of s_memtime (against the 100 MHz wall clock stamped next to it)
eng.step(20); torch.cuda.synchronize()
for rep in range(3):
    eng.step(1); torch.cuda.synchronize()
    lib.reart_debug_phase_clock(buf)
    v = list(buf)
    for w, name, n in ((0, "fwd", 6), (1, "bwd_block", 9)):
        ts = v[16 * w:16 * w + n]
        wall = (v[16 * w + 13] - v[16 * w + 12]) * 1e-2           # us between the first and the latest stamp (100 MHz wall clock)
        if wall > 0:
            TICK_US = wall / (ts[n - 1] - ts[0])
            print(f"{name}: s_memtime runs at {1e-3 / TICK_US:.3f} GHz here ({ts[n - 1] - ts[0]} ticks in {wall:.2f} us)")
        if w == 1:
            # stamps 0..3 are thread 0's (tile loads | a. dw | b. softmax backward, ds complete); behind stamp 3 the waves split by
            # role and each role stamps its own end: 4 gR|gt tile (wave 0), 5 gW2 tile (first wave that has one), 6 / 7 hidden
            # gradient dp, then gW1 / gb1 (first wave of that role); 8 after a closing barrier = the slower role
            us = lambda k0, k1: (ts[k1] - ts[k0]) * TICK_US
            print(f"bwd_block (us): tile loads {us(0, 1):.2f} | a. dw {us(1, 2):.2f} | b. ds {us(2, 3):.2f} | roles side by side from stamp 3: "
                  f"gR|gt tile ends +{us(3, 4):.2f}, gW2 tile ends +{us(3, 5):.2f}, dp ends +{us(3, 6):.2f}, gW1/gb1 end +{us(3, 7):.2f}, "
                  f"all waves done +{us(3, 8):.2f} | total {us(0, 8):.2f} us: the lifetime of ONE workgroup (block 1)")
            if v[16 + 9] and v[16 + 11]:
                # inside "tile loads" (thread 0): 9 all loads issued, 10 loads returned (the diagnostic build waits there), 11 LDS stores issued
                pt = v[16:32]
                d = lambda k0, k1: (pt[k1] - pt[k0]) * TICK_US
                print(f"bwd_block tile loads (us): loads issued {d(0, 9):.2f} | loads returned {d(9, 10):.2f} | stores done {d(10, 11):.2f} | "
                      f"barrier {d(11, 1):.2f}")
            continue
        print(name, "deltas (s_memtime ticks):", [ts[i + 1] - ts[i] for i in range(n - 1)], "total", ts[n - 1] - ts[0],
              f"= {(ts[n - 1] - ts[0]) * TICK_US:.2f} us: the lifetime of ONE workgroup (block 1)")
    fz = v[8:16]          # [0][8] body workgroup 1 entry, [9] its end; [10] bookkeeping workgroup (the last one) entry, [14] its end
    print(f"finalize: body workgroup 1 (column sums, Gram-Schmidt backward, Adam) lifetime {(fz[1] - fz[0]) * TICK_US:.2f} us | bookkeeping "
          f"workgroup (loss partials, pow / sqrt / temperature on a wave each, one barrier, the stores) lifetime {(fz[6] - fz[2]) * TICK_US:.2f} us "
          f"(the two run on different XCDs, whose counters are not comparable: lifetimes only)")
    if hasattr(lib, "reart_debug_post_clock"):
        lib.reart_debug_post_clock(pbuf)
        p = list(pbuf)
        print("post_kernel, one workgroup of each kind (lifetime, us): flow blend %.2f | Chamfer gradient %.2f | launch order %.2f | profile %.2f; "
              "(kernel durations by rocprofv3: profiles/*kernel_stats_clean.csv)" % tuple([(p[2 * k + 1] - p[2 * k]) * TICK_US for k in range(4)]))
