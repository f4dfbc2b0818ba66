"""Host-side contract of the PointNet++ layer surface (no GPU): which shapes the fused chain serves, the refusals that are
decided from arguments alone, and the names the mirrored module exports."""
import pytest

INVALID_ARG, UNSUPPORTED = -1, -2   # REART_ERR_INVALID_ARG, REART_ERR_UNSUPPORTED (include/reart_hip.h)
P = 4096                            # a non-null dummy address: these calls are refused before anything is launched


def L():
    from reart_amd import _lib

    return _lib.lib()


# (D, K, C1, C2, C3, rows, xyz_first) -> served by reart_mlp_chain
SERVES = [
    ((6, 32, 32, 32, 64, 1024, 0), 1), ((0, 16, 32, 32, 64, 128, 0), 1), ((0, 16, 32, 32, 64, 128, 1), 1),
    ((131, 64, 128, 128, 256, 16384, 1), 1), ((512, 128, 256, 256, 256, 128, 0), 1), ((323, 128, 128, 196, 256, 1280, 0), 1),
    ((3, 16, 64, 4, 32, 256, 0), 1), ((259, 128, 256, 252, 256, 128, 1), 1),
    # the five tuples the older kernels own (features first): still theirs
    ((3, 32, 32, 32, 64, 1024, 0), 0), ((3, 64, 64, 64, 128, 1024, 0), 0), ((3, 128, 64, 96, 128, 1024, 0), 0),
    ((320, 64, 128, 128, 256, 1024, 0), 0), ((320, 128, 128, 196, 256, 1024, 0), 0), ((8, 64, 128, 128, 256, 1024, 0), 0),
    # ... but not their neighbours: another D, the other column order, another group size
    ((6, 64, 64, 64, 128, 1024, 0), 1), ((3, 32, 32, 32, 64, 1024, 1), 1), ((322, 64, 128, 128, 256, 1024, 0), 1),
    ((320, 64, 128, 128, 256, 1024, 1), 1), ((3, 16, 32, 32, 64, 1024, 0), 1), ((320, 128, 128, 128, 256, 1024, 0), 1),
    # each bound's first refused value
    ((-1, 32, 32, 32, 64, 1024, 0), 0), ((513, 32, 32, 32, 64, 1024, 0), 0),
    ((6, 8, 32, 32, 64, 1024, 0), 0), ((6, 24, 32, 32, 64, 1152, 0), 0), ((6, 48, 32, 32, 64, 768, 0), 0), ((6, 256, 32, 32, 64, 1024, 0), 0),
    ((6, 32, 0, 32, 64, 1024, 0), 0), ((6, 32, 33, 32, 64, 1024, 0), 0), ((6, 32, 48, 32, 64, 1024, 0), 0), ((6, 32, 288, 32, 64, 1024, 0), 0),
    ((6, 32, 32, 0, 64, 1024, 0), 0), ((6, 32, 32, 6, 64, 1024, 0), 0), ((6, 32, 32, 260, 64, 1024, 0), 0),
    ((6, 32, 32, 32, 0, 1024, 0), 0), ((6, 32, 32, 32, 80, 1024, 0), 0), ((6, 32, 32, 32, 288, 1024, 0), 0),
    ((6, 32, 32, 32, 64, 0, 0), 0), ((6, 32, 32, 32, 64, 64, 0), 0), ((6, 32, 32, 32, 64, 1056, 0), 0),
    ((6, 32, 32, 32, 64, 1024, 2), 0), ((6, 32, 32, 32, 64, 1024, -1), 0),
]


@pytest.mark.parametrize("shape,served", SERVES)
def test_chain_serves_table(shape, served):
    assert L().reart_mlp_chain_serves(*shape) == served, shape


def test_routing_keeps_the_older_kernels_shapes():
    """The Python layer asks the same predicate; the tuples it sends to reart_mlp_chain3 / _wide are the ones refused here."""
    from reart_amd.networks import feature_extractor as fe

    for (C1, C2, C3, K) in fe.CHAIN3:
        assert not fe.chain_serves(3, K, (C1, C2, C3), 1024, 0)
    for (C1, C2, C3, K) in fe.CHAIN3_WIDE:
        assert not fe.chain_serves(320, K, (C1, C2, C3), 1024, 0)
    assert fe.chain_serves(6, 32, (32, 32, 64), 1024, 0)
    assert not fe.chain_serves(6, 32, (32, 32), 1024, 0) and not fe.chain_serves(6, 32, (32, 32, 64, 64), 1024, 0)


def chain(idx=P, K=32, S=4, Npts=64, F=P, D=6, Q=P, C=P, xyz_first=0, W1=P, b1=P, C1=32, W2=P, b2=P, C2=32, W3=P, b3=P, C3=64,
          rows=1024, Y=P, ldy=64, ycol0=0, ws=P, ws_bytes=None):
    lib = L()
    if ws_bytes is None:
        ws_bytes = lib.reart_mlp_chain_workspace_bytes(D, C1, C2, C3)
    return lib.reart_mlp_chain(idx, K, S, Npts, F, D, Q, C, xyz_first, W1, b1, C1, W2, b2, C2, W3, b3, C3, rows, Y, ldy, ycol0, ws, ws_bytes, None)


def test_chain_refusals_decided_from_arguments():
    lib = L()
    need = lib.reart_mlp_chain_workspace_bytes(6, 32, 32, 64)
    assert need == 4 * 32 * 4 * (9 + 32 + 32) and need % 16 == 0          # three images [Cin][32][4]
    assert lib.reart_mlp_chain_workspace_bytes(6, 32, 32, 256) == 4 * 32 * 8 * (9 + 32 + 32)    # a wide layer: [Cin][32][8]
    assert lib.reart_mlp_chain_workspace_bytes(6, 32, 32, 257) == 0 and lib.reart_mlp_chain_workspace_bytes(-1, 32, 32, 64) == 0
    assert chain(rows=0) == 0                                               # an empty problem is fine
    for null in ("idx", "Q", "F", "W1", "b1", "W2", "b2", "W3", "b3", "Y"):
        assert chain(**{null: None}) == INVALID_ARG, null
    assert chain(F=None, D=0, ws_bytes=0) == INVALID_ARG                    # D = 0 needs no F: refused for its workspace only
    assert chain(ws=None) == INVALID_ARG
    assert chain(ws_bytes=need - 1) == INVALID_ARG                          # a workspace that is too small
    assert chain(ws=P + 4) == INVALID_ARG                                   # ... or not 16-byte aligned
    assert chain(ldy=63) == INVALID_ARG and chain(ycol0=-1) == INVALID_ARG and chain(ycol0=1) == INVALID_ARG
    assert chain(rows=-128) == INVALID_ARG and chain(K=0) == INVALID_ARG and chain(D=-1) == INVALID_ARG
    assert chain(K=48, rows=1000) == INVALID_ARG                            # rows % K
    # well-formed, but not a shape of this kernel: status UNSUPPORTED, the caller goes layer by layer
    assert chain(D=3) == UNSUPPORTED                                        # reart_mlp_chain3's
    assert chain(K=48, rows=768) == UNSUPPORTED and chain(rows=1056) == UNSUPPORTED
    assert chain(C1=48) == UNSUPPORTED and chain(C3=288, ldy=288) == UNSUPPORTED and chain(D=513) == UNSUPPORTED


def layer(X=P, ldx=8, idx=None, K=0, S=0, Npts=0, F=None, D=0, Q=None, C=None, xyz_first=0, Wt=P, bias=P, rows=1200, Cin=8, Cout=8,
          relu=1, pool_k=0, Y=P, ldy=8, ycol0=0):
    return L().reart_mlp_layer(X, ldx, idx, K, S, Npts, F, D, Q, C, xyz_first, Wt, bias, rows, Cin, Cout, relu, pool_k, Y, ldy, ycol0, None)


def test_widened_layer_refusals_decided_from_arguments():
    for pool_k in (7, 32, 64, 128, 384, 1201):                              # rows % pool_k != 0: every group size alike
        assert layer(pool_k=pool_k, rows=1200) == INVALID_ARG, pool_k
    assert layer(pool_k=-1) == INVALID_ARG
    for pool_k in (0, 1, 16, 24, 100, 384):                                 # null pointers come before the group size
        assert layer(pool_k=pool_k, Wt=None) == INVALID_ARG and layer(pool_k=pool_k, Y=None) == INVALID_ARG
        assert layer(pool_k=pool_k, X=None) == INVALID_ARG
        assert layer(pool_k=pool_k, idx=P, K=24, S=50, Npts=9, D=5, F=None, Q=P) == INVALID_ARG      # D > 0 without F
        assert layer(pool_k=pool_k, idx=P, K=24, S=50, Npts=9, D=5, F=P, Q=None) == INVALID_ARG
    assert layer(pool_k=24, rows=0) == 0


def test_public_names_of_the_mirrored_module():
    import torch.nn as nn

    from reart_amd.networks import feature_extractor as fe
    from reart_amd.networks import pointnet2_utils as pu

    for name in ("index_points", "farthest_point_sample", "query_ball_point", "square_distance", "sample_and_group",
                 "sample_and_group_all", "PointNetSetAbstraction", "PointNetSetAbstractionMsg", "PointNetFeaturePropagation"):
        assert callable(getattr(pu, name)), name
    for cls in (pu.PointNetSetAbstraction, pu.PointNetSetAbstractionMsg, pu.PointNetFeaturePropagation):
        assert issubclass(cls, nn.Module)
    assert fe._SAMsg is pu.PointNetSetAbstractionMsg and fe._FP is pu.PointNetFeaturePropagation
    assert issubclass(fe._SAAll, pu.PointNetSetAbstraction) and callable(fe.rec_freeze)
    model = fe.PointNet2Msg2(out_dim=64, normal_channel=True)              # no longer refused
    assert model.sa1.conv_blocks[0][0].weight.shape[1] == 9 and model.fp1.mlp_convs[0].weight.shape[1] == 137
    assert isinstance(model.sa3, pu.PointNetSetAbstraction) and model.sa3.group_all
    plain = fe.PointNet2Msg2(out_dim=64)
    assert plain.sa1.conv_blocks[0][0].weight.shape[1] == 6 and plain.fp1.mlp_convs[0].weight.shape[1] == 134
