"""Writes tests/golden/workspace_sizes.json: what every *_workspace_bytes entry point of libreart_hip.so returns over a fixed
table of shapes.  tests/test_workspace_sizes_cpu.py holds the library under test to these figures entry for entry.

The file is a record of ONE commit: it is generated once, from a build of the commit in front of a change to the workspace
layouts, and never from the tree that change is tested in.  Usage (in a checkout of that commit, after building it):

    python tests/golden/make_golden_workspace_sizes.py <commit id>

No GPU is needed: the size queries are host code."""
import ctypes
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "workspace_sizes.json")

# the assignment solvers (include/reart_hip.h: n <= 4096 plain / race / mc, <= REART_LAP_LARGE_MAX_N = 8192 large forms;
# racers <= 28)
LAP_N = (1, 15, 16, 511, 512, 1024, 2048, 2049, 4096, 4097, 8192, 8193)
LAP_B = (0, 1, 19, 95)
LAP_RACERS = (1, 2, 13, 28, 29)


def lap_shapes():
    return [list(s) for s in itertools.product(LAP_B, LAP_N)] + [[-1, 512], [19, 0]]


def lap_race_shapes():
    return [list(s) for s in itertools.product(LAP_B, LAP_N, LAP_RACERS)] + [[19, 1024, 0], [-1, 1024, 2]]


def _knn3():
    """(N, P1, P2, K) of the D = 3 searches: K <= 16 in registers (rounded up to 1, 2, 3, 4, 8, 16), 17 ... 1024 in a list
    in LDS; target lengths around the multiples of 16, 64 and 256; enough queries for every slice count."""
    s = [[10, 4096, 4096, 1], [1, 1, 1, 1], [0, 8, 8, 1], [1, 0, 8, 1], [1, 8, 0, 1], [1, 8, 8, 0]]
    for P2 in (15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 19200):
        for K in (1, 3):
            s.append([1, 300, P2, K])
            s.append([19, 4096, P2, K])
    for K in (2, 4, 5, 8, 9, 16, 17, 64, 65, 128, 129, 256, 512, 513, 1024, 1025):
        s.append([2, 500, 1500, K])
    s += [[1, 64, 100000, 1], [1, 100000, 64, 3], [640, 64, 64, 1], [19, 4096, 512, 3]]
    return s


def _knn_d():
    """(N, P1, P2, D, K) of the any-D searches: 1 <= D <= 256, 1 <= K <= 1024."""
    s = [[c[0], c[1], c[2], 3, c[3]] for c in _knn3()[:12]]
    for D in (1, 2, 4, 63, 64, 65, 256, 257, 0):
        for K in (1, 3, 16, 17, 128, 1024, 1025):
            s.append([2, 500, 1500, D, K])
    for P2 in (1, 15, 16, 17, 63, 64, 65, 255, 256, 257):
        s.append([3, 77, P2, 5, 4])
        s.append([1, 1, P2, 64, 1])
    s += [[0, 8, 8, 4, 1], [1, 0, 8, 4, 1], [1, 8, 0, 4, 1], [1, 8, 8, 4, 0], [1, 100000, 64, 8, 1], [4096, 4096, 64, 2, 1]]
    return s


def _relax():
    """reart_relax_config fields that differ from the base case (tests/test_boundary_cpu.py's, at the headline shape)."""
    s = [dict()]                                               # headline: N 4096, P 20, B 19, H 128, flow on
    s.append(dict(N=1, P=1, B=1, H=1, M_max=3, M_total=3))     # smallest
    for flags in itertools.product((0, 1), (0, 1), (0, 1)):
        s.append(dict(use_flow=flags[0], use_grid=flags[1], profile=flags[2]))
    s += [dict(P=32), dict(P=33), dict(P=0), dict(N=0), dict(B=0), dict(H=0), dict(flow_k=2), dict(M_max=2)]
    s += [dict(B=1024, M_total=1024 * 64), dict(B=1025, M_total=1025 * 64)]
    s += [dict(tune_long=1), dict(tune_long=1, N=2048, B=299, H=64, M_total=299 * 64), dict(B=300, P=20, H=128, N=1000, M_total=300 * 64)]
    for N in (15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4097, 19200):
        s.append(dict(N=N))
    for M in (3, 15, 16, 17, 63, 64, 65, 255, 256, 257, 2049):
        s.append(dict(M_max=M, M_total=19 * M))
    s += [dict(search_mode=1), dict(use_boxes=0), dict(tune_slices=1), dict(tune_slices=4, tune_slices_flow=2), dict(tune_cloud=2),
          dict(search_mode=1, N=300, B=3, M_total=192), dict(use_boxes=0, N=100000, B=2, M_total=128), dict(use_assign=1, use_flow=0)]
    return s


def relax_config(over):
    from reart_amd import relax

    cfg = relax.RelaxConfig(N=4096, P=20, B=19, H=128, cano_idx=1, use_flow=1, flow_k=3, M_max=64, M_total=19 * 64, n_iter=100, ring=8,
                            lambda_flow=1.0, trans_lr=1e-2, seg_lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, start_tau=1.0,
                            end_tau=0.1, use_boxes=1, lambda_assign=1.0)
    for k, v in over.items():
        setattr(cfg, k, v)
    return cfg


def _around(*limits):
    out = []
    for v in limits:
        out += [v - 1, v, v + 1]
    return out


SHAPES = {
    "reart_knn_points_workspace_bytes": _knn3(),
    "reart_knn_points_workspace_bytes_d": _knn_d(),
    "reart_knn_points_workspace_bytes_f64": _knn_d(),
    "reart_knn_points_backward_workspace_bytes":
        [[10, 4096, 4096, 1], [1, 1, 1, 1], [0, 8, 8, 1], [-1, 8, 8, 1], [1, 0, 0, 1], [1, 8, 8, 0], [1, -1, 8, 1], [1, 8, -1, 1],
         [2, 500, 1500, 16], [2, 500, 1500, 1024], [3, 17, 63, 3], [3, 65, 257, 5]],
    "reart_chamfer_bidir_workspace_bytes":
        [[N, P] for N in (0, 1, 10, 19, 640) for P in (0, 1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 2048, 4096, 19200)],
    "reart_blend_anchor_motion_workspace_bytes":
        [[4096, 64, 3], [1, 1, 1], [0, 64, 3], [64, 0, 3], [64, 64, 0], [64, 64, 16], [64, 64, 17]] +
        [[nq, nr, 3] for nq in (15, 16, 17, 63, 64, 65, 255, 256, 257) for nr in (3, 15, 16, 17, 63, 64, 65, 255, 256, 257)],
    "reart_blend_anchor_motion_batch_workspace_bytes":
        [[19, 4096, 64, 3], [1, 1, 1, 1], [0, 64, 64, 3], [1, 0, 64, 3], [1, 64, 0, 3], [1, 64, 64, 0], [9, 2048, 64, 16], [9, 2048, 64, 17]] +
        [[B, nq, nr, 3] for B in (1, 9, 19) for nq in (15, 17, 63, 65, 255, 257, 4096) for nr in (3, 16, 17, 64, 65, 256, 257)],
    "reart_kin_post_workspace_bytes":
        [[9, 2048, 64, 3], [19, 4096, 64, 3], [1, 1, 0, 0], [1, 1, 1, 1], [0, 64, 64, 3], [9, 0, 64, 3], [9, 2048, 0, 3], [9, 2048, 64, 0],
         [9, 2048, -1, -1]] +
        [[B, N, nr, 3] for B in (1, 9) for N in (15, 16, 17, 63, 64, 65, 255, 256, 257, 1000) for nr in (0, 3, 17, 64, 257)],
    "reart_flow_loss_workspace_bytes": [[]],
    "reart_base_backward_workspace_bytes":
        [[4096, 20, 19, 128], [1, 1, 1, 1], [0, 20, 19, 128], [4096, 0, 19, 128], [4096, 20, 0, 128], [4096, 20, 19, 0],
         [4096, 32, 19, 128], [4096, 33, 19, 128], [2048, 20, 1024, 64], [2048, 20, 1025, 64]] +
        [[N, P, B, 16] for N in (15, 16, 17, 63, 64, 65, 255, 256, 257, 19200) for P, B in ((4, 3), (10, 9), (20, 19))],
    "reart_compute_pc_transform_backward_workspace_bytes":
        [[4096, 20, 19], [0, 1, 1], [-1, 1, 1], [4096, 0, 19], [4096, 20, 0], [100, 1024, 3], [100, 1025, 3], [100, 7, 1024], [100, 7, 1025]] +
        [[64, P, B] for P in (1, 3, 16, 17, 64) for B in (1, 5, 16, 19)],
    "reart_base_backward_cano_workspace_bytes":
        [[20, 19], [1, 1], [0, 19], [20, 0], [20, 1024], [20, 1025]] + [[P, 9] for P in _around(32, 64, 1024)] +
        [[P, B] for P in (1, 3, 16, 17) for B in (1, 5, 16, 21)],
    "reart_fk_backward_workspace_bytes":
        [[20, 19, 19], [1, 1, 0], [0, 19, 19], [20, 0, 19], [20, 19, -1], [20, 19, 0], [64, 19, 63], [65, 19, 64], [8, 1024, 7], [8, 1025, 7]] +
        [[P, B, E] for P in (2, 5, 16, 17) for B in (1, 9, 16, 43) for E in (1, 10, 11, 16)],
    "reart_mlp_chain3_wide_workspace_bytes":
        [[0, 64, 64, 128], [3, 64, 64, 128], [1, 1, 1, 1], [0, 1, 1, 1], [3, 0, 64, 64], [3, 64, 0, 64], [3, 64, 64, 0]] +
        [[D, C, C, C2] for D in (3, 6, 13, 61, 125, 253) for C in (15, 16, 17, 64, 128, 256, 257) for C2 in (32, 129, 256, 257)],
    "reart_mlp_chain_workspace_bytes":
        [[0, 64, 64, 128], [3, 64, 64, 128], [0, 1, 1, 1], [-1, 1, 1, 1], [3, 0, 64, 64], [3, 64, 0, 64], [3, 64, 64, 0]] +
        [[D, C, C, C2] for D in (0, 3, 6, 13, 61, 125, 253) for C in (15, 16, 17, 64, 128, 129, 256, 257) for C2 in (32, 129, 256, 257)],
    "reart_three_interpolate_workspace_bytes":
        [[10, 4096, 1024], [1, 1, 1], [0, 64, 64], [1, 0, 64], [1, 64, 0], [1, 64, 3]] +
        [[B, N, 16] for B in (1, 3, 10) for N in (15, 16, 17, 21, 22, 63, 64, 65, 255, 256, 257)],
    "reart_grid_knn_workspace_bytes":
        [[19, 4096], [1, 1], [0, 64], [1, 0]] + [[E, Nt] for E in (1, 3, 19) for Nt in (15, 16, 17, 63, 64, 65, 255, 256, 257, 19200)],
    "reart_knn_points_warm_workspace_bytes":
        [[19, 4096, 4096, 1], [19, 4096, 64, 3], [1, 1, 1, 1], [0, 8, 8, 1], [1, 0, 8, 1], [1, 8, 0, 1], [-1, 8, 8, 1], [1, 8, 8, 2],
         [1, 8, 8, 0], [1, 8, 8, 4]] +
        [[N, P1, P2, K] for N in (1, 19) for P1 in (17, 64, 300) for P2 in (15, 16, 17, 63, 64, 65, 255, 256, 257) for K in (1, 3)],
    "reart_chamfer_loss_workspace_bytes":
        [[19, 4096, 4096], [1, 1, 1], [0, 8, 8], [1, 0, 8], [1, 8, 0], [65535, 8, 8], [65536, 8, 8], [4, 1 << 28, 8], [1, 1 << 30, 8]] +
        [[N, P1, P2] for N in (1, 19) for P1 in (15, 17, 64, 255, 257, 4096) for P2 in (15, 16, 17, 63, 64, 65, 255, 256, 257)],
    "reart_flow_term_workspace_bytes":
        [[19, 4096, 64], [1, 1, 3], [0, 64, 64], [1, 0, 64], [1, 64, 2], [1024, 64, 64], [1025, 64, 64], [1, 1 << 20, 3],
         [1, (1 << 20) + 1, 3], [1, 64, 1 << 20], [1, 64, (1 << 20) + 1], [64, 1 << 20, 3], [65, 1 << 20, 3]] +
        [[B, N, nr] for B in (1, 9, 19) for N in (15, 17, 255, 256, 257, 2048) for nr in (3, 15, 16, 17, 63, 64, 65, 255, 256, 257)],
    "reart_lap_workspace_bytes": lap_shapes(),
    "reart_lap_large_workspace_bytes": lap_shapes(),
    "reart_lap_resolve_large_workspace_bytes": lap_shapes(),
    "reart_lap_race_workspace_bytes": lap_race_shapes(),
    "reart_lap_mc_workspace_bytes": lap_race_shapes(),
    "reart_match_smnn_workspace_bytes":
        [[19, 512, 512], [1, 1, 1], [0, 8, 8], [1, 0, 8], [1, 8, 0]] +
        [[E, NA, NB] for E in (1, 3, 19) for NA in (15, 16, 17, 31, 32, 33, 63, 64, 65) for NB in (7, 8, 9, 32, 255, 256, 257)],
    "reart_screw_fit_workspace_bytes": [[19, 400], [1, 1], [0, 0], [19, 0], [19, -1], [20, 4096], [20, 4097]],
    "reart_structure_term_workspace_bytes":
        [[20, 20, 190], [1, 1, 0], [0, 4, 4], [20, 0, 4], [20, 4, -1]] +
        [[T, P, E] for T in (1, 5, 64, 65, 256, 257, 1024, 1025) for P in (2, 64, 65) for E in (0, 1, 3, 32, 33, 4096, 4097)],
    "reart_rel_trans_backward_workspace_bytes":
        [[20, 20, 190], [1, 1, 0], [0, 4, 4], [20, 0, 4], [20, 4, -1]] +
        [[T, P, E] for T in (1, 5, 64, 65, 256, 257, 1024, 1025) for P in (2, 64, 65) for E in (0, 1, 3, 32, 33, 4096, 4097)],
    "reart_connection_select_workspace_bytes":
        [[4096, 20, 19, 10], [1, 1, 0, 1], [0, 4, 4, 4], [64, 0, 4, 4], [64, 4, -1, 4], [64, 4, 4, 0]] +
        [[N, P, E, k] for N in (1, 63, 64, 65, 255, 257, 5000, 65536, 65537) for P in (2, 64, 65) for E in (0, 3, 4096, 4097)
         for k in (1, 10, 64, 65)],
    "reart_connection_term_workspace_bytes":
        [[20, 4096, 19, 10], [1, 1, 0, 1], [0, 4, 4, 4], [4, 0, 4, 4], [4, 4, -1, 4], [4, 4, 4, 0]] +
        [[T, N, E, k] for T in (1, 1024, 1025) for N in (1, 62, 63, 64, 65, 255, 257, 65536, 65537) for E in (0, 3, 4, 4096, 4097)
         for k in (1, 8, 10, 64, 65)],
    "reart_relax_workspace_bytes": _relax(),
}


def collect():
    """{entry point: [[arguments, bytes], ...]} from the library the package loads."""
    sys.path.insert(0, ROOT)
    from reart_amd import _lib, relax

    L = _lib.lib()
    names = sorted(n for n in _lib.PROTOTYPES if "workspace_bytes" in n)
    assert names == sorted(SHAPES), sorted(set(names) ^ set(SHAPES))
    out = {}
    for name in names:
        rows = []
        for args in SHAPES[name]:
            if name == "reart_relax_workspace_bytes":
                cfg = relax_config(args)
                got = relax._lib_fns().reart_relax_workspace_bytes(ctypes.byref(cfg))
            else:
                got = getattr(L, name)(*args)
            rows.append([args, int(got)])
        out[name] = rows
    return out


if __name__ == "__main__":
    commit = sys.argv[1]
    sizes = collect()
    with open(OUT, "w") as f:
        json.dump({"commit": commit, "sizes": sizes}, f, separators=(",", ":"))
        f.write("\n")
    print(OUT, sum(len(v) for v in sizes.values()), "entries from", len(sizes), "entry points")
