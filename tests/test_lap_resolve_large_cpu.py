"""Argument checks of the large warm re-solve (reart_lap_resolve_large_workspace_bytes, reart_lap_resolve_large): they come
before any device call, so they run without a GPU."""
OK, INVALID_ARG = 0, -1   # REART_OK, REART_ERR_INVALID_ARG (include/reart_hip.h)


def test_resolve_large_workspace_bytes():
    from reart_amd import _lib

    L = _lib.lib()
    size = L.reart_lap_resolve_large_workspace_bytes
    assert size(3, 0) == 0
    assert size(3, 1) > 0
    assert size(3, 8192) > size(3, 4097) > 0
    assert size(3, 8193) == 0
    assert size(-1, 5) == 0
    # the re-solve's pass results and the row potentials come on top of the potentials and the diagnostics
    assert size(3, 4097) >= 3 * 4097 * (8 + 8 + 8 + 4 + 8) + 3 * 16
    # the entries below the limit keep theirs
    assert L.reart_lap_workspace_bytes(3, 4097) == 0


def test_resolve_large_rejects_bad_arguments_without_a_gpu():
    from reart_amd import _lib

    L = _lib.lib()
    p = 4096                # stands for a device address: a rejected call reads nothing
    n, B = 5, 2
    need = L.reart_lap_resolve_large_workspace_bytes(B, n)
    solve = L.reart_lap_resolve_large
    assert solve(p, 1, 8193, 0, p, p, p, p, p, 1 << 40, None) == INVALID_ARG        # n above the limit
    assert solve(p, 1, 0, 0, p, p, p, p, p, 1 << 40, None) == INVALID_ARG
    assert solve(p, -1, n, 0, p, p, p, p, p, need, None) == INVALID_ARG
    assert solve(None, B, n, 0, p, p, p, p, p, need, None) == INVALID_ARG            # cost
    assert solve(p, B, n, 0, None, p, p, p, p, need, None) == INVALID_ARG            # col4row
    assert solve(p, B, n, 0, p, None, p, p, p, need, None) == INVALID_ARG            # certified
    assert solve(p, B, n, 0, p, p, None, p, p, need, None) == INVALID_ARG            # price_in
    assert solve(p, B, n, 0, p, p, p, None, p, need, None) == INVALID_ARG            # price_out
    assert solve(p, B, n, 0, p, p, p, p, None, need, None) == INVALID_ARG            # no workspace
    assert solve(p, B, n, 0, p, p, p, p, p, need - 1, None) == INVALID_ARG           # short workspace
    assert solve(p, B, n, 7, p, p, p, p, p, 0, None) == INVALID_ARG                  # (whatever the step limit)
    # an empty batch is fine, whatever else is passed
    assert solve(None, 0, n, 0, None, None, None, None, None, 0, None) == OK
    assert solve(None, 0, 8192, -3, None, None, None, None, None, 0, None) == OK


def test_resolve_below_the_limit_keeps_its_limit():
    from reart_amd import _lib

    L = _lib.lib()
    assert L.reart_lap_resolve(None, 1, 5000, None, None, None, None, None, 0, None) == INVALID_ARG
    p = 4096
    assert L.reart_lap_resolve(p, 1, 5000, p, p, p, p, p, 1 << 40, None) == INVALID_ARG
