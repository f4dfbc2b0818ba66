"""Argument checks of the large assignment entry points (reart_lap_large_workspace_bytes, reart_lap_auction_large):
they come before any device call, so they run without a GPU."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID_ARG = 0, -1   # REART_OK, REART_ERR_INVALID_ARG (include/reart_hip.h)


def test_large_limit_in_the_header_is_the_bindings():
    from reart_amd import _lib

    text = open(os.path.join(ROOT, "include", "reart_hip.h")).read()
    m = re.search(r"^#define\s+REART_LAP_LARGE_MAX_N\s+(\d+)\s*$", text, flags=re.M)
    assert m is not None
    assert int(m.group(1)) == _lib.LAP_LARGE_MAX_N == 8192


def test_large_workspace_bytes():
    from reart_amd import _lib

    L = _lib.lib()
    assert L.reart_lap_large_workspace_bytes(3, 8192) > L.reart_lap_large_workspace_bytes(3, 4097) > 0
    assert L.reart_lap_large_workspace_bytes(3, 8193) == 0
    assert L.reart_lap_large_workspace_bytes(3, 0) == 0
    assert L.reart_lap_large_workspace_bytes(-1, 5) == 0
    # the entry takes every size from 1 up; the entries below the limit keep theirs
    assert L.reart_lap_large_workspace_bytes(3, 1) > 0
    assert L.reart_lap_workspace_bytes(3, 4097) == 0


def test_large_auction_rejects_bad_arguments_without_a_gpu():
    from reart_amd import _lib

    L = _lib.lib()
    p = 4096                # stands for a device address: a rejected call reads nothing
    n, B = 5, 2
    need = L.reart_lap_large_workspace_bytes(B, n)
    solve = L.reart_lap_auction_large
    assert solve(p, None, None, 1, 8193, p, p, p, p, 1 << 40, None) == INVALID_ARG        # n above the limit
    assert solve(p, None, None, 1, 0, p, p, p, p, 1 << 40, None) == INVALID_ARG
    assert solve(p, None, None, -1, n, p, p, p, p, need, None) == INVALID_ARG
    assert solve(None, None, None, B, n, p, p, p, p, need, None) == INVALID_ARG            # cost
    assert solve(p, None, None, B, n, None, p, p, p, need, None) == INVALID_ARG            # col4row
    assert solve(p, None, None, B, n, p, None, p, p, need, None) == INVALID_ARG            # certified
    assert solve(p, None, None, B, n, p, p, None, p, need, None) == INVALID_ARG            # price_out
    assert solve(p, p, None, B, n, p, p, p, p, need, None) == INVALID_ARG                  # src without tgt
    assert solve(p, None, p, B, n, p, p, p, p, need, None) == INVALID_ARG                  # tgt without src
    assert solve(p, None, None, B, n, p, p, p, p, need - 1, None) == INVALID_ARG           # short workspace
    assert solve(p, None, None, B, n, p, p, p, None, need, None) == INVALID_ARG            # no workspace
    # an empty batch is fine, whatever else is passed
    assert solve(None, None, None, 0, n, None, None, None, None, 0, None) == OK
    assert solve(None, None, None, 0, 8192, None, None, None, None, 0, None) == OK
    # the entries below the limit are as they were
    assert L.reart_lap_auction(None, 1, 5000, None, None, None, None, None, 0, None) == INVALID_ARG
