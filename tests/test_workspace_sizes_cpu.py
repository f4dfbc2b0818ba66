"""Every *_workspace_bytes entry point returns what tests/golden/workspace_sizes.json records for it, and the assignment
solvers' statistics words stay at the offset the host reads them from.  Host code only: no device is touched.

The golden file was written by tests/golden/make_golden_workspace_sizes.py from a build of the commit it names (the one in
front of the change that derives every size and every workspace pointer from one walk), never from the tree under test."""
import ctypes
import importlib.util
import itertools
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def _maker():
    spec = importlib.util.spec_from_file_location("make_golden_workspace_sizes",
                                                  os.path.join(HERE, "golden", "make_golden_workspace_sizes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


MAKER = _maker()
GOLDEN = json.load(open(os.path.join(HERE, "golden", "workspace_sizes.json")))


def test_golden_covers_every_size_entry_point():
    from reart_amd import _lib

    names = sorted(n for n in _lib.PROTOTYPES if "workspace_bytes" in n)
    assert len(names) == 32
    assert sorted(GOLDEN["sizes"]) == names
    assert len(GOLDEN["commit"]) >= 7
    for name in names:      # the recorded shapes are the table's, in its order
        assert [row[0] for row in GOLDEN["sizes"][name]] == json.loads(json.dumps(MAKER.SHAPES[name])), name


@pytest.mark.parametrize("name", sorted(GOLDEN["sizes"]))
def test_sizes_are_the_recorded_ones(name):
    from reart_amd import _lib, relax

    L = _lib.lib()
    rows = GOLDEN["sizes"][name]
    assert len(rows) >= 1
    for args, want in rows:
        if name == "reart_relax_workspace_bytes":
            cfg = MAKER.relax_config(args)
            got = relax._lib_fns().reart_relax_workspace_bytes(ctypes.byref(cfg))
        else:
            got = getattr(L, name)(*args)
        assert got == want, (name, args, got, want)


def test_statistics_words_stay_where_the_host_reads_them():
    """The diagnostics block [B][4] follows the potentials [B][n] f64, rounded up to 256 bytes: the formula of the commit
    the golden file names, as a literal.  Beyond the largest n any solver takes the query answers 0, as the sizes do."""
    from reart_amd import _lib
    from reart_amd.utils import lap

    L = _lib.lib()
    for B, n in itertools.product(MAKER.LAP_B, MAKER.LAP_N):
        want = ((8 * B * n + 255) // 256) * 256 if n <= _lib.LAP_LARGE_MAX_N else 0
        assert L.reart_lap_stats_offset(B, n) == want, (B, n)
        assert lap.stats_words(B, n) == want, (B, n)
    assert L.reart_lap_stats_offset(-1, 512) == 0
    assert L.reart_lap_stats_offset(19, 0) == 0
