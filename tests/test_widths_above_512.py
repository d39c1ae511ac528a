"""MLPs wider than the fused kernels (hid, dout or a source width above nlam_max_width() = 512) on the tiled-GEMM family
(nlam_mlp_fwd_gemm / nlam_mlp_bwd_gemm): the C-ABI as host logic, then make_mlp MLPs, GNN layers, models and the trainer
against the oracle on the GPU.  Bars: max|a-b| / max|b| <= 1e-4 for outputs and every gradient."""
import ctypes as C
import re
from pathlib import Path

import pytest
import torch

from conftest import rel_err

ROOT = Path(__file__).resolve().parent.parent
TOL = 1e-4
GEMM_SYMBOLS = ["nlam_mlp_fwd_gemm", "nlam_mlp_bwd_gemm", "nlam_mlp_fwd_gemm_workspace_floats",
                "nlam_mlp_bwd_gemm_workspace_floats", "nlam_mlp_bwd_gemm_blocks"]
FAKE = 0x1000   # a non-null address: the argument checks below return before any launch could touch it


def _lib():
    from neural_lam_amd import _lib as L

    return L, L.load()


# ---------------------------------------------------------------- host logic (no GPU) ----------------------------------------


def test_gemm_entry_points_are_declared_and_exported():
    from neural_lam_amd import _lib as L

    header = (ROOT / "include" / "nlam_hip.h").read_text()
    declared = set(re.findall(r"^int(?:32|64)_t\s+(nlam_\w+)\s*\(", header, flags=re.M))
    lib = L.load()
    for name in GEMM_SYMBOLS:
        assert name in declared and name in L.EXPORTS and hasattr(lib, name), name
    assert lib.nlam_max_width() == 512 and L.ABI_VERSION == 8


def _fwd(L, widths=(768, 768, 768), hid=768, dout=768, batch=1, rows=1000, flags=0):
    p = L.MlpFwd()
    p.nsrc, p.batch, p.rows, p.ntiles = len(widths), batch, rows, (rows + 31) // 32
    for k, w in enumerate(widths):
        p.src[k].ptr, p.src[k].width, p.src[k].bstride = FAKE, w, rows * w
    p.W1, p.b1, p.W2, p.b2 = FAKE, FAKE, FAKE, FAKE
    p.hid, p.dout, p.flags, p.eps = hid, dout, flags, 1e-5
    p.out, p.out_bstride = FAKE, rows * dout
    return p


def _bwd(L, widths=(768, 768, 768), hid=768, dout=768, batch=1, rows=1000, dmode=(1, 1, 1), flags=0):
    p = L.MlpBwd()
    p.nsrc, p.batch, p.rows, p.ntiles = len(widths), batch, rows, (rows + 31) // 32
    for k, w in enumerate(widths):
        p.src[k].ptr, p.src[k].width, p.src[k].bstride = FAKE, w, rows * w
        p.dmode[k], p.dsrc[k], p.dsrc_bstride[k] = dmode[k], FAKE, rows * w
    p.W1, p.W2, p.hid, p.dout, p.flags = FAKE, FAKE, hid, dout, flags
    p.g_out, p.out_bstride, p.z1, p.dz1, p.dz2, p.rowptr = FAKE, rows * dout, FAKE, FAKE, FAKE, FAKE
    return p


def test_gemm_arguments_are_rejected_before_any_launch():
    L, lib = _lib()
    EINVAL, EUNSUP = -1, -2
    null = C.c_void_p(0)
    assert lib.nlam_mlp_fwd_gemm(None, null) == EINVAL and lib.nlam_mlp_bwd_gemm(None, null) == EINVAL
    assert lib.nlam_mlp_fwd_gemm_workspace_floats(None) == EINVAL and lib.nlam_mlp_bwd_gemm_workspace_floats(None) == EINVAL
    cases = []
    p = _fwd(L); p.src[1].ptr = None; cases.append((p, EINVAL))                     # null source
    p = _fwd(L); p.W2 = None; cases.append((p, EINVAL))                             # null weight
    p = _fwd(L); p.hid = 0; cases.append((p, EINVAL))                               # no hidden width
    p = _fwd(L); p.src[2].width = 0; cases.append((p, EINVAL))
    p = _fwd(L, widths=(768,), flags=L.F_ADD_SRC1); cases.append((p, EINVAL))      # residual of a source that is not there
    p = _fwd(L, widths=(640, 768), flags=L.F_ADD_SRC0); cases.append((p, EINVAL))  # residual width != dout
    p = _fwd(L); p.ldw1 = 100; cases.append((p, EINVAL))                            # W1 rows shorter than the sources
    p = _fwd(L); p.aggr = FAKE; p.nseg_total = 10; cases.append((p, EINVAL))         # aggregation without row pointers
    p = _fwd(L); p.wpack, p.wpack_floats = None, 0; cases.append((p, EINVAL))        # no scratch for the intermediates
    p = _fwd(L, flags=L.F_PRE_ADD); cases.append((p, EUNSUP))                       # factorised edge MLP: not this family
    p = _fwd(L); p.ncat = 2; cases.append((p, EUNSUP))
    for p, rc in cases:
        assert lib.nlam_mlp_fwd_gemm(C.byref(p), null) == rc
    cases = []
    p = _bwd(L); p.dz1 = None; cases.append((p, EINVAL))
    p = _bwd(L); p.dmode[1] = 4; cases.append((p, EINVAL))
    p = _bwd(L); p.dsrc[0] = None; cases.append((p, EINVAL))
    p = _bwd(L); p.dz2_ld = 800; cases.append((p, EINVAL))
    p = _bwd(L); p.ln_w = FAKE; cases.append((p, EINVAL))                            # LayerNorm without xhat / rstd
    p = _bwd(L); p.g_aggr = FAKE; p.nseg_total = 5; cases.append((p, EINVAL))        # no receiver of each row
    p = _bwd(L); p.vec_partials, p.vec_partials_rows, p.vec_stride = FAKE, 8, 768; cases.append((p, EINVAL))
    p = _bwd(L, flags=L.F_ACC_DSRC0); cases.append((p, EUNSUP))
    for p, rc in cases:
        assert lib.nlam_mlp_bwd_gemm(C.byref(p), null) == rc


def test_gemm_workspace_queries():
    L, lib = _lib()
    B, rows = 2, 1000
    p = _fwd(L, batch=B, rows=rows, widths=(3,), hid=1000, dout=600)
    assert lib.nlam_mlp_fwd_gemm_workspace_floats(C.byref(p)) == B * rows * (600 + 1000)   # z2 / messages + z1 (not saved)
    p.z1 = FAKE
    assert lib.nlam_mlp_fwd_gemm_workspace_floats(C.byref(p)) == B * rows * 600
    q = _bwd(L, batch=B, rows=rows, widths=(768, 768, 768), dmode=(1, 2, 3))
    assert lib.nlam_mlp_bwd_gemm_workspace_floats(C.byref(q)) == B * rows * 768               # staging of the mode-3 gradient
    q.ln_w, q.xhat, q.rstd = FAKE, FAKE, FAKE
    assert lib.nlam_mlp_bwd_gemm_workspace_floats(C.byref(q)) == 2 * B * rows * 768           # + the upstream gradient rows
    q.dmode[2] = 0
    assert lib.nlam_mlp_bwd_gemm_workspace_floats(C.byref(q)) == B * rows * 768
    assert lib.nlam_mlp_bwd_gemm_blocks(C.byref(q)) >= 1
    q.flags = L.F_PRE_ADD
    assert lib.nlam_mlp_bwd_gemm_workspace_floats(C.byref(q)) == -2
    # the fused entry points keep refusing these widths
    assert lib.nlam_mlp_fwd(C.byref(_fwd(L)), C.c_void_p(0)) == -2


def test_routing_above_the_fused_width_is_host_logic():
    from neural_lam_amd import gnn_layers as hl
    from neural_lam_amd import ops

    L, lib = _lib()
    assert not ops.uses_gemm_family(512, 512, [512, 512, 512])
    assert not ops.uses_gemm_family(64, 17, [3])
    assert ops.uses_gemm_family(513, 64, [64])
    assert ops.uses_gemm_family(64, 600, [3])
    assert ops.uses_gemm_family(64, 64, [1000])
    # chunked layers above 512 run their chunks one by one (never ChunkedMLPFunction); at 512 the chunked path stays
    assert not hl.SplitMLPs([hl.make_mlp([1152, 576, 576]) for _ in range(2)], [3, 4]).fully_fused
    assert hl.SplitMLPs([hl.make_mlp([1024, 512, 512]) for _ in range(2)], [3, 4]).fully_fused   # (two 512-wide sources in the layers)
    # the factorised edge MLP has no kernel above 512: the layer takes the unfactorised route
    for d in (576, 768, 1024):
        q = L.MlpFwd()
        q.nsrc, q.batch, q.rows, q.ntiles = 3, 1, 57616, 1801
        for k in range(3):
            q.src[k].width = d
        q.hid, q.dout, q.flags = d, d, L.F_PRE_ADD | (3 << 8)
        assert lib.nlam_pre_add_supported(C.byref(q)) == 0, d


# ---------------------------------------------------------------- GPU ------------------------------------------------------


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from neural_lam_amd import _lib

    _lib.load()
    return torch.device("cuda:0")


def _rand_ei(ns, nr, e, seed):
    g = torch.Generator().manual_seed(seed)
    ei = torch.stack([torch.randint(0, ns, (e,), generator=g), torch.randint(0, nr, (e,), generator=g)])
    ei[1, -1] = nr - 1   # the oracle takes the receiver count from the edge index
    return ei


def _check_grads(net, ref, tol=TOL):
    rp = dict(ref.named_parameters())
    for k, p in net.named_parameters():
        q = rp[k]
        if q.grad is None:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
            continue
        assert p.grad is not None, k
        assert rel_err(p.grad.cpu(), q.grad) < tol, (k, rel_err(p.grad.cpu(), q.grad))


@pytest.mark.gpu
@pytest.mark.parametrize("batch", ["1", "2", "shared"])
@pytest.mark.parametrize("hidden_layers", [0, 1, 2])
@pytest.mark.parametrize("ln", [True, False])
@pytest.mark.parametrize("kin,hid,dout", [(3, 768, 768), (1536, 640, 640), (3072, 1024, 1024), (600, 600, 1000)])
def test_make_mlp_matches_oracle(dev, kin, hid, dout, ln, hidden_layers, batch):
    from neural_lam_amd import gnn_layers as hl
    from oracle import gnn_layers as og

    torch.manual_seed(kin + hid)
    blueprint = [kin] + [hid] * hidden_layers + [dout]
    ref = og.make_mlp(blueprint, layer_norm=ln)
    net = hl.make_mlp(blueprint, layer_norm=ln)
    net.load_state_dict(ref.state_dict())
    net.to(dev)
    rows = 301
    if batch == "shared":   # one copy read by both batch items (stride 0, expand_to_batch)
        base = torch.randn(rows, kin)
        x1 = base.clone().requires_grad_()
        x2 = base.to(dev).requires_grad_()
        y1, y2 = ref(x1.expand(2, rows, kin)), net(x2.expand(2, rows, kin))
    else:
        x = torch.randn(int(batch), rows, kin)
        x1, x2 = x.clone().requires_grad_(), x.to(dev).requires_grad_()
        y1, y2 = ref(x1), net(x2)
    assert rel_err(y2.cpu(), y1) < TOL
    y1.sin().sum().backward()
    y2.sin().sum().backward()
    assert rel_err(x2.grad.cpu(), x1.grad) < TOL
    _check_grads(net, ref)


def _layer_case(dev, cls_name, d, ns, nr, e, B=2, seed=0, same=False, one_pass=False, **kw):
    from neural_lam_amd import gnn_layers as hl
    from oracle import gnn_layers as og

    ei = _rand_ei(ns, nr, e, seed=seed + d)
    torch.manual_seed(seed + d)
    ref = getattr(og, cls_name)(ei, d, **kw)
    net = getattr(hl, cls_name)(ei, d, **kw)
    net.load_state_dict(ref.state_dict())
    net.to(dev)
    send, rec, edge = torch.randn(B, ns, d), torch.randn(B, nr, d), torch.randn(B, e, d)
    r1, e1 = rec.clone().requires_grad_(), edge.clone().requires_grad_()
    r2, e2 = rec.to(dev).requires_grad_(), edge.to(dev).requires_grad_()
    if same:   # the same tensor as sender and receiver (mesh <-> mesh)
        s1, s2 = r1, r2
    else:
        s1, s2 = send.clone().requires_grad_(), send.to(dev).requires_grad_()
    o1, o2 = ref(s1, r1, e1), net(s2, r2, e2)
    if one_pass:   # the schedule really has NLAM_TILE_SPLIT tiles (atomic partial sums), no virtual segments
        assert net._host_csr[2] and net._host_csr[0].comb_ptr is None
    o1 = o1 if isinstance(o1, tuple) else (o1,)
    o2 = o2 if isinstance(o2, tuple) else (o2,)
    for a, b in zip(o2, o1):
        assert rel_err(a.cpu(), b) < TOL
    sum((o * o).sum() for o in o1).backward()
    sum((o * o).sum() for o in o2).backward()
    pairs = ((r2, r1), (e2, e1)) if same else ((s2, s1), (r2, r1), (e2, e1))
    for a, b in pairs:
        assert rel_err(a.grad.cpu(), b.grad) < TOL
    _check_grads(net, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("update_edges", [True, False])
@pytest.mark.parametrize("aggr", ["sum", "mean"])
@pytest.mark.parametrize("cls_name", ["InteractionNet", "PropagationNet"])
@pytest.mark.parametrize("d", [576, 768, 1024])
def test_layers_above_512_match_oracle(dev, cls_name, d, aggr, update_edges):
    _layer_case(dev, cls_name, d, 61, 47, 501, update_edges=update_edges, aggr=aggr)


@pytest.mark.gpu
@pytest.mark.parametrize("cls_name,d,ns,nr,e,same", [
    ("InteractionNet", 576, 40, 7, 1500, False),     # in-degree ~214: receivers split over several tiles
    ("PropagationNet", 768, 5, 300, 1400, False),    # most receivers without edges, mean aggregation, sender residual
    ("InteractionNet", 1024, 300, 300, 5, False),    # almost every node isolated
    ("InteractionNet", 576, 90, 90, 700, True),      # the same tensor as sender and receiver
    ("PropagationNet", 640, 33, 65, 2081, True),
])
def test_layers_above_512_on_awkward_graphs(dev, cls_name, d, ns, nr, e, same):
    _layer_case(dev, cls_name, d, ns, nr, e, seed=e, same=same)


@pytest.mark.gpu
@pytest.mark.parametrize("cls_name,d", [("InteractionNet", 576), ("PropagationNet", 768)])
def test_one_pass_split_schedule_above_512(dev, monkeypatch, cls_name, d):
    """graph.VIRTUAL_SPLIT = False: receivers of in-degree ~214 are cut into NLAM_TILE_SPLIT pieces that each add the sum of their
    own rows -- forward aggregation and receiver gradients (dmode 3) against the oracle."""
    from neural_lam_amd import graph as G

    monkeypatch.setattr(G, "VIRTUAL_SPLIT", False)
    _layer_case(dev, cls_name, d, 40, 7, 1500, seed=7, one_pass=True)


@pytest.mark.gpu
def test_launch_without_rows_writes_zero_aggregates_and_gradients(dev):
    """An edge set without edges whose receivers the tile schedule still covers: the aggregate, the segment-summed receiver
    gradient and the bias partial sums come out as zeros (the buffers start as NaN)."""
    from neural_lam_amd import graph as G

    L, lib = _lib()
    d, nseg = 600, 5
    rowptr = torch.zeros(nseg + 1, dtype=torch.int32)
    tiles, _, _ = G.build_tile_schedule(rowptr)
    tiles, rowptr = tiles.to(dev), rowptr.to(dev)
    W1, b1, W2, b2 = (torch.randn(*s_, device=dev) for s_ in ((d, 3 * d), (d,), (d, d), (d,)))
    srcs = [torch.randn(1, 4, d, device=dev) for _ in range(3)]
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = L.MlpFwd()
    p.nsrc, p.batch, p.rows, p.ntiles, p.tiles = 3, 1, 0, int(tiles.shape[0]), tiles.data_ptr()
    for k, t in enumerate(srcs):
        p.src[k].ptr, p.src[k].width, p.src[k].bstride = t.data_ptr(), d, 4 * d
    p.W1, p.b1, p.W2, p.b2 = W1.data_ptr(), b1.data_ptr(), W2.data_ptr(), b2.data_ptr()
    p.hid, p.dout, p.eps = d, d, 1e-5
    aggr = torch.full((1, nseg, d), float("nan"), device=dev)
    p.aggr, p.rowptr, p.nseg_total = aggr.data_ptr(), rowptr.data_ptr(), nseg
    assert lib.nlam_mlp_fwd_gemm_workspace_floats(C.byref(p)) == 0
    assert lib.nlam_mlp_fwd_gemm(C.byref(p), stream) == 0
    q = L.MlpBwd()
    q.nsrc, q.batch, q.rows, q.ntiles, q.tiles = 3, 1, 0, int(tiles.shape[0]), tiles.data_ptr()
    for k, t in enumerate(srcs):
        q.src[k].ptr, q.src[k].width, q.src[k].bstride = t.data_ptr(), d, 4 * d
    q.W1, q.W2, q.hid, q.dout, q.nseg_total = W1.data_ptr(), W2.data_ptr(), d, d, nseg
    dummy = torch.zeros(1, device=dev)
    g_aggr, seg_of_row = torch.zeros(1, nseg, d, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    q.g_aggr, q.seg_of_row, q.rowptr = g_aggr.data_ptr(), seg_of_row.data_ptr(), rowptr.data_ptr()
    q.z1, q.dz1, q.dz2 = dummy.data_ptr(), dummy.data_ptr(), dummy.data_ptr()
    drec = torch.full((1, nseg, d), float("nan"), device=dev)
    q.dmode[2], q.dsrc[2], q.dsrc_bstride[2] = 3, drec.data_ptr(), nseg * d
    nblk, vs = lib.nlam_mlp_bwd_gemm_blocks(C.byref(q)), 640
    vecp = torch.full((nblk, 4, vs), float("nan"), device=dev)
    q.vec_partials, q.vec_partials_rows, q.vec_stride = vecp.data_ptr(), nblk, vs
    assert lib.nlam_mlp_bwd_gemm_workspace_floats(C.byref(q)) == 0
    assert lib.nlam_mlp_bwd_gemm(C.byref(q), stream) == 0
    torch.cuda.synchronize()
    assert bool((aggr == 0).all()) and bool((drec == 0).all()) and bool((vecp == 0).all())


def _meps_m2m(dev, d, seed=0):
    """An m2m-size edge set: 57 616 edges among 10 000 mesh nodes, senders = receivers (the node table)."""
    from neural_lam_amd import gnn_layers as hl

    ei = _rand_ei(10_000, 10_000, 57_616, seed=seed)
    torch.manual_seed(seed)
    net = hl.InteractionNet(ei, d).to(dev)
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.randn(1, 10_000, d, device=dev, generator=g)
    e = torch.randn(1, 57_616, d, device=dev, generator=g)
    return ei, net, x, e


@pytest.mark.gpu
def test_meps_size_m2m_layer_matches_oracle_on_gpu_and_is_bit_reproducible(dev):
    from oracle import gnn_layers as og

    d = 768
    ei, net, x, e = _meps_m2m(dev, d)
    ref = og.InteractionNet(ei, d).to(dev)
    ref.load_state_dict(net.state_dict())

    def run(m):
        xr, er = x.clone().requires_grad_(), e.clone().requires_grad_()
        m.zero_grad(set_to_none=True)
        outs = m(xr, xr, er)
        sum((o * o).sum() for o in outs).backward()
        return [o.detach() for o in outs], xr.grad, er.grad, {k: p.grad.clone() for k, p in m.named_parameters()}

    o_ref, gx_ref, ge_ref, gp_ref = run(ref)
    o1, gx1, ge1, gp1 = run(net)
    for a, b in zip(o1, o_ref):
        assert rel_err(a, b) < TOL
    assert rel_err(gx1, gx_ref) < TOL and rel_err(ge1, ge_ref) < TOL
    for k in gp1:
        assert rel_err(gp1[k], gp_ref[k]) < TOL, k
    o2, gx2, ge2, gp2 = run(net)   # a second run: bit-identical
    for a, b in zip(o1, o2):
        assert torch.equal(a, b)
    assert torch.equal(gx1, gx2) and torch.equal(ge1, ge2)
    for k in gp1:
        assert torch.equal(gp1[k], gp2[k]), k


def _graph(ds, hierarchical=False):
    from neural_lam_amd import graph as G

    ext = ds.get_xy_extent("state")
    raw = G.create_regular_grid_graph(ds.get_xy("state"), hierarchical=hierarchical)
    return G.normalise_graph(raw, max(ext[1] - ext[0], ext[3] - ext[2])), raw


def _datastore(tmp_path):
    from neural_lam_amd.datastore import SyntheticDatastore

    return SyntheticDatastore(30, 27, 5, 2, 1, root_path=tmp_path, boundary="random", seed=1)


@pytest.mark.gpu
@pytest.mark.parametrize("cls_name,d", [("GraphLAM", 640), ("HiLAM", 576), ("HiLAMParallel", 576)])
def test_training_step_above_512_matches_oracle(dev, tmp_path, cls_name, d):
    from neural_lam_amd import models as hm
    from oracle import models as om

    ds = _datastore(tmp_path)
    graph, _ = _graph(ds, hierarchical=cls_name != "GraphLAM")
    kw = dict(hidden_dim=d, processor_layers=2)
    torch.manual_seed(3)
    o_fc = om.ARForecaster(getattr(om, cls_name)(ds, graph, **kw), ds)
    h_fc = hm.ARForecaster(getattr(hm, cls_name)(ds, graph=graph, **kw), ds)
    h_fc.load_state_dict(o_fc.state_dict())
    step = hm.ForecasterStep(h_fc, ds).to(dev)
    N = ds.num_grid_points
    g = torch.Generator().manual_seed(4)
    init, target, forcing = torch.randn(1, 2, N, 5, generator=g), torch.randn(1, 2, N, 5, generator=g), torch.randn(1, 2, N, 6, generator=g)
    o_pred, o_loss = om.training_loss(o_fc, (init, target, forcing), om.per_var_std_uniform(ds), om.interior_mask_bool(ds))
    o_loss.backward()
    h_pred, h_loss = step(init.to(dev), target.to(dev), forcing.to(dev))
    h_loss.backward()
    assert abs(float(h_loss.detach()) - float(o_loss.detach())) < TOL * abs(float(o_loss.detach()))
    assert rel_err(h_pred.cpu(), o_pred) < TOL
    _check_grads(h_fc, o_fc)


@pytest.mark.gpu
def test_graph_efm_above_512_rolls_out(dev, tmp_path):
    from neural_lam_amd import graph as G
    from neural_lam_amd import graph_efm
    from neural_lam_amd import models as hm

    ds = _datastore(tmp_path)
    _, raw = _graph(ds)
    G.save_graph(tmp_path / "graph" / "ms", raw)
    torch.manual_seed(0)
    model = graph_efm.GraphEFMMultiScale(ds, graph_name="ms", hidden_dim=576, prior_m2m_layers=1, encoder_m2m_layers=1,
                                         decoder_m2m_layers=1)
    fc = hm.ARForecaster(model, ds).to(dev)
    N = ds.num_grid_points
    g = torch.Generator().manual_seed(0)
    init, target, forcing = (torch.randn(1, 2, N, 5, generator=g).to(dev), torch.randn(1, 2, N, 5, generator=g).to(dev),
                             torch.randn(1, 2, N, 6, generator=g).to(dev))
    pred, _ = fc(init, forcing, target)
    assert pred.shape == (1, 2, N, 5) and bool(torch.isfinite(pred).all())
    pred.square().sum().backward()
    without = [k for k, p in model.named_parameters() if p.grad is None]
    # the variational encoder and the embedder of the current state feed the training-time posterior only
    assert all(k.startswith(("encoder.", "grid_current_embedder.")) for k in without), without
    assert all(bool(torch.isfinite(p.grad).all()) for p in model.parameters() if p.grad is not None)
    assert model.mesh_embedder[0].weight.grad is not None


def _trainer_setup(dev, tmp_path, d=640, T=2):
    from neural_lam_amd import models as hm
    from oracle import models as om

    ds = _datastore(tmp_path)
    graph, _ = _graph(ds)
    torch.manual_seed(7)
    o_fc = om.ARForecaster(om.GraphLAM(ds, graph, hidden_dim=d, processor_layers=2), ds)
    h_fc = hm.ARForecaster(hm.GraphLAM(ds, graph=graph, hidden_dim=d, processor_layers=2), ds)
    h_fc.load_state_dict(o_fc.state_dict())
    step = hm.ForecasterStep(h_fc, ds).to(dev)
    N = ds.num_grid_points
    g = torch.Generator().manual_seed(8)
    batch = (torch.randn(1, 2, N, 5, generator=g), torch.randn(1, T, N, 5, generator=g), torch.randn(1, T, N, 6, generator=g))
    return ds, o_fc, h_fc, step, batch


@pytest.mark.gpu
def test_trainer_adamw_trajectory_above_512_matches_oracle(dev, tmp_path):
    from neural_lam_amd.trainer import Trainer
    from oracle import models as om

    ds, o_fc, h_fc, step, batch_cpu = _trainer_setup(dev, tmp_path)
    batch = tuple(t.to(dev) for t in batch_cpu)
    pvs, mask = om.per_var_std_uniform(ds), om.interior_mask_bool(ds)
    opt = torch.optim.AdamW(o_fc.parameters(), lr=1e-3, betas=(0.9, 0.95))
    tr = Trainer(step, lr=1e-3, use_graph=True)
    for it in range(3):
        opt.zero_grad(set_to_none=True)
        _, o_loss = om.training_loss(o_fc, batch_cpu, pvs, mask)
        o_loss.backward()
        opt.step()
        h_loss = tr.step(*batch)
        assert abs(float(h_loss) - float(o_loss)) < TOL * abs(float(o_loss)), it
    assert tr._graph is not None
    o_sd = o_fc.state_dict()
    for k, v in h_fc.state_dict().items():
        if v.numel():
            assert float((v.cpu() - o_sd[k]).abs().max()) < 2e-4, k


@pytest.mark.gpu
def test_trainer_graph_step_equals_eager_step_above_512(dev, tmp_path):
    from neural_lam_amd.trainer import Trainer

    results = []
    for use_graph in (False, True):
        _, _, h_fc, step, batch_cpu = _trainer_setup(dev, tmp_path / str(use_graph))
        batch = tuple(t.to(dev) for t in batch_cpu)
        tr = Trainer(step, lr=1e-3, use_graph=use_graph)
        losses = [float(tr.step(*batch)) for _ in range(2)]
        torch.cuda.synchronize()
        results.append((losses, {k: v.detach().cpu().clone() for k, v in h_fc.state_dict().items()}))
    (l_e, sd_e), (l_g, sd_g) = results
    assert l_e == l_g
    for k in sd_e:
        assert torch.equal(sd_e[k], sd_g[k]), k


@pytest.mark.gpu
def test_rollout_backward_twice_leaves_no_pending_hand_over(dev, tmp_path):
    from neural_lam_amd import ops

    _, _, h_fc, step, batch_cpu = _trainer_setup(dev, tmp_path, T=3)
    batch = tuple(t.to(dev) for t in batch_cpu)
    grads = []
    for _ in range(2):
        h_fc.zero_grad(set_to_none=True)
        _, loss = step(*batch)
        loss.backward()
        ops.rollout_shared_reset()   # raises if a backward left a held-back gradient behind
        grads.append({k: p.grad.clone() for k, p in h_fc.named_parameters() if p.grad is not None})
    assert grads[0].keys() == grads[1].keys() and len(grads[0]) > 0
    for k in grads[0]:
        assert torch.equal(grads[0][k], grads[1][k]), k


def _run_layer(net, args, cots, autocast=False):
    """Outputs, input gradients and parameter gradients of one layer call back-propagated with fixed cotangents."""
    xs = [a.clone().requires_grad_() for a in args]
    net.zero_grad(set_to_none=True)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        outs = net(*xs)
    outs = outs if isinstance(outs, tuple) else (outs,)
    sum((o.float() * c).sum() for o, c in zip(outs, cots)).backward()
    return ([o.detach().float().cpu() for o in outs], [x.grad.detach().float().cpu() for x in xs],
            {k: p.grad.detach().float().cpu() for k, p in net.named_parameters()})


def _wgrad_plan(mm_flags, m, widths, rows):
    L, lib = _lib()
    q = L.Wgrad()
    q.A, q.m, q.batch, q.rows, q.nsrc, q.flags, q.n = FAKE, m, 1, rows, len(widths), mm_flags, sum(widths)
    for k, w in enumerate(widths):
        q.src[k].ptr, q.src[k].width, q.src[k].bstride = FAKE, w, rows * w
    q.partials, q.nparts = FAKE, lib.nlam_wgrad_nparts(C.byref(q))
    return lib.nlam_wgrad_plan(C.byref(q))


def _layer_pair(dev, cls_name, d, ns, nr, e, seed):
    from neural_lam_amd import gnn_layers as hl
    from oracle import gnn_layers as og

    ei = _rand_ei(ns, nr, e, seed=seed)
    torch.manual_seed(seed)
    ref = getattr(og, cls_name)(ei, d)
    net = getattr(hl, cls_name)(ei, d)
    net.load_state_dict(ref.state_dict())
    g = torch.Generator().manual_seed(seed)
    args = [torch.randn(1, n, d, generator=g) for n in (ns, nr, e)]
    return ref, net.to(dev), args


@pytest.mark.gpu
@pytest.mark.parametrize("cls_name,d", [("InteractionNet", 768), ("PropagationNet", 1024)])
def test_f32_matrix_mode_backward_above_512(dev, cls_name, d):
    """Matrix mode "f32" (served by three bf16 terms in the tiled-GEMM family; weight gradients on the fp32-MFMA plan WGP_WIDE):
    outputs, input gradients and every parameter gradient against the oracle; the forward also against bf16x3."""
    from neural_lam_amd import _lib as L
    from neural_lam_amd import ops

    ns, nr, e = 200, 150, 3000
    assert _wgrad_plan(0, d, [d, d, d], e) == L.WGP_WIDE and _wgrad_plan(L.F_SILU_B, d, [d], e) == L.WGP_WIDE
    ref, net, args = _layer_pair(dev, cls_name, d, ns, nr, e, seed=d)
    cots = [torch.randn(1, nr, d), torch.randn(1, e, d)]
    o_ref, gx_ref, gp_ref = _run_layer(ref, args, cots)
    old = ops.MATMUL_MODE
    try:
        ops.set_matmul_mode("f32")
        o32, gx32, gp32 = _run_layer(net, [a.to(dev) for a in args], [c.to(dev) for c in cots])
        ops.set_matmul_mode("bf16x3")
        o3, _, _ = _run_layer(net, [a.to(dev) for a in args], [c.to(dev) for c in cots])
    finally:
        ops.set_matmul_mode(old)
    for a, b, c in zip(o32, o_ref, o3):
        assert rel_err(a, b) < TOL and rel_err(a, c) < TOL
    for a, b in zip(gx32, gx_ref):
        assert rel_err(a, b) < TOL
    for k in gp_ref:
        assert rel_err(gp32[k], gp_ref[k]) < TOL, (k, rel_err(gp32[k], gp_ref[k]))


BF16_NOISE_FACTOR = 1.5   # the bar of tests/test_full_size_parity.py: HIP under autocast at most this much noisier than the
BF16_NOISE_FLOOR = 1e-3   # reference under autocast (both against the fp32 reference), plus this allowance


def _rel_l2(a, b):
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    assert bool(torch.isfinite(a).all())
    return float((a - b).norm() / b.norm().clamp(min=1e-30))


@pytest.mark.gpu
@pytest.mark.parametrize("cls_name,d", [("InteractionNet", 768), ("PropagationNet", 1024)])
def test_bf16_autocast_noise_above_512_is_not_above_the_reference(dev, cls_name, d):
    """bf16 autocast (one-term kernels: gemm_kernel<1, *>, weight gradients on the one-term plan WGP_LDMA_1): per output, input
    gradient and parameter gradient, err(HIP under autocast vs fp32 oracle) <= 1.5 x err(oracle under autocast vs fp32 oracle)
    + 1e-3, the oracle run on the GPU."""
    from neural_lam_amd import _lib as L

    ns, nr, e = 200, 150, 3000
    assert _wgrad_plan(1 << 8, d, [d, d, d], e) == L.WGP_LDMA_1 and _wgrad_plan((1 << 8) | L.F_SILU_B, d, [d], e) == L.WGP_LDMA_1
    ref, net, args = _layer_pair(dev, cls_name, d, ns, nr, e, seed=d + 1)
    ref = ref.to(dev)
    g = torch.Generator().manual_seed(5)
    cots = [torch.randn(1, nr, d, generator=g).to(dev), torch.randn(1, e, d, generator=g).to(dev)]
    args = [a.to(dev) for a in args]
    o32, gx32, gp32 = _run_layer(ref, args, cots)
    o_amp, gx_amp, gp_amp = _run_layer(ref, args, cots, autocast=True)
    o_hip, gx_hip, gp_hip = _run_layer(net, args, cots, autocast=True)
    for h, r, f in zip(o_hip, o_amp, o32):
        assert rel_err(h, f) <= BF16_NOISE_FACTOR * rel_err(r, f) + BF16_NOISE_FLOOR, (rel_err(h, f), rel_err(r, f))
    for h, r, f in zip(gx_hip, gx_amp, gx32):
        assert _rel_l2(h, f) <= BF16_NOISE_FACTOR * _rel_l2(r, f) + BF16_NOISE_FLOOR, (_rel_l2(h, f), _rel_l2(r, f))
    for k in gp32:
        e_h, e_r = _rel_l2(gp_hip[k], gp32[k]), _rel_l2(gp_amp[k], gp32[k])
        assert e_h <= BF16_NOISE_FACTOR * e_r + BF16_NOISE_FLOOR, (k, e_h, e_r)


@pytest.mark.gpu
@pytest.mark.parametrize("d", [256, 512])
def test_gemm_family_agrees_with_fused_family(dev, d, monkeypatch):
    """A/B through the C-ABI: the same layer with the routing threshold lowered, so that its launches run on
    nlam_mlp_*_gemm, against the fused kernels (bf16x3 on both sides)."""
    from neural_lam_amd import gnn_layers as hl
    from neural_lam_amd import ops

    ei = _rand_ei(300, 200, 4000, seed=d)
    torch.manual_seed(d)
    net = hl.InteractionNet(ei, d).to(dev)
    g = torch.Generator().manual_seed(d)
    send, rec, edge = (torch.randn(2, n, d, generator=g).to(dev) for n in (300, 200, 4000))
    res = []
    for threshold in (512, d // 2):
        monkeypatch.setattr(ops, "_MAX_FUSED", threshold)
        net.zero_grad(set_to_none=True)
        xs = [t.clone().requires_grad_() for t in (send, rec, edge)]
        outs = net(*xs)
        sum((o * o).sum() for o in outs).backward()
        res.append(([o.detach() for o in outs], [x.grad for x in xs], {k: p.grad.clone() for k, p in net.named_parameters()}))
    (o_f, gx_f, gp_f), (o_g, gx_g, gp_g) = res
    for a, b in zip(o_g, o_f):
        assert rel_err(a, b) < 1e-5
    for a, b in zip(gx_g, gx_f):
        assert rel_err(a, b) < 1e-5
    for k in gp_f:
        assert rel_err(gp_g[k], gp_f[k]) < 1e-5, k
