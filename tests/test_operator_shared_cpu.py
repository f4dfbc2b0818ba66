"""No GPU: the inputs of tests/test_operator_shared_parent_gpu.py make its equal bits a statement about the order of the inverse
lists (csrc/invlist_dev.h)."""
import numpy as np

from tests import test_operator_shared_parent_gpu as T


def _f32_sum(rows):
    acc = np.zeros(rows.shape[1], np.float32)
    for r in rows:
        acc = acc + r
    return acc


def test_pile_sums_depend_on_the_order():
    """What makes the equal bits above a statement about the ORDER of the inverse lists: for every pile-up point of the
    connection, layer and interpolation cases the float32 sum of its contributions in ascending record order (the lists'
    contract) differs in at least one bit from the sum in descending order.  Were the sums insensitive, a builder that
    placed a point's records in another order would still give the parent's bits.  `_pile_both` has equal contributions
    (one source, one target) and is left out: it pins counts and offsets only."""
    piles = []
    for n in T.CONN:
        if T.CONN[n][4] in ("tgt", "src"):
            piles += [(n, *p) for p in T.conn_pile_contributions(n)]
    for n in T.LAYER:
        if T.LAYER[n][3] is not None:
            piles += [(n, *p) for p in T.layer_pile_contributions(n)]
    piles += [("interp_n90_s5", *p) for p in T.interp_pile_contributions("interp_n90_s5")]
    assert len(piles) == 3 + 4 + 10                    # three connection piles, two clouds of two layer cases, 2 x 5 coarse points
    for case, point, rows in piles:
        rows = np.ascontiguousarray(rows, np.float32)
        assert len(rows) >= 24, (case, point, len(rows))                   # dozens of records on the point
        up, down = _f32_sum(rows), _f32_sum(rows[::-1])
        assert not np.array_equal(T.bits(up), T.bits(down)), f"{case}, {point}: {len(rows)} contributions add up alike in both orders"
