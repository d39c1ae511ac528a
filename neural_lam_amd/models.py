"""Step predictors, autoregressive rollout and training step on the HIP layers.

Host-side mirror of the reference's model files for the hot path only
(SURVEY.md §8a); every MLP / GNN layer below is a ``libnlam_hip.so`` kernel,
the surrounding glue (feature concat, rescale, boundary mix, loss) is stock
PyTorch-ROCm elementwise work.

Reference -> here (same class / argument / attribute / parameter names):
  StepPredictor      models/step_predictors/base.py:15-396
  BaseGraphModel     models/step_predictors/graph/base.py:31-344
  GraphLAM           models/step_predictors/graph/graph_lam.py:28-188
  BaseHiGraphModel   models/step_predictors/graph/hierarchical.py:30-292
  HiLAM              models/step_predictors/graph/hi_lam.py:25-376
  HiLAMParallel      models/step_predictors/graph/hi_lam_parallel.py:24-218
  ARForecaster       models/forecasters/autoregressive.py:14-149
  wmse               metrics.py:37-137
  mse .. get_metric  metrics.py:10-34, 140-394 (mse, mae, wmae, nll, crps_gauss: evaluation formulas)
  ForecasterStep     the training_step / loss / AdamW lines of models/module.py:293-304, 326-417, 463-510
  ForecasterStep.evaluate  validation_step / test_step, models/module.py:546-576, 607-681 (epoch ends: evaluation.py)

Differences that do not change results: the graph may be handed in pre-loaded
(``graph=``) instead of being read from ``datastore.root_path``; the
input-independent embeddings (g2m / m2g / m2m / mesh embedders) are computed
once per rollout instead of once per AR step (``static_cache``); the final
processor layer does not materialise the edge output the reference discards
(graph_lam.py:185).
"""
from __future__ import annotations

import contextlib

import torch
from torch import nn

from . import graph as G
from .gnn_layers import GNNSequential, InteractionNet, get_gnn_class, make_mlp


def inverse_softplus(x, beta=1.0, threshold=20.0):
    """utils/tensor.py:7-51."""
    x_clamped = torch.clamp(x, min=torch.log(torch.tensor(1e-6 + 1)) / beta, max=threshold / beta)
    non_linear = torch.log(torch.expm1(x_clamped * beta)) / beta
    return torch.where(x * beta <= threshold, non_linear, x)


def inverse_sigmoid(x):
    """utils/tensor.py:53-81."""
    xc = torch.clamp(x, min=1e-6, max=1 - 1e-6)
    return torch.log(xc / (1 - xc))


# nlam_affine_mix for the elementwise tail of a step (A/B on one box: +3 % forecast rate, +1 % training rate)
FUSED_STATE_UPDATE = True
# the torch.cat of the grid input features folded into grid_embedder (ops.CatMLPFunction); NLAM_FOLD_CAT=0 for A/B runs
import os as _os

FOLD_INPUT_CAT = _os.environ.get("NLAM_FOLD_CAT", "1") == "1"
# the ensemble CRPS term of EFMForecasterStep(crps_members=M) on ops.CrpsEnsFunction; NLAM_FUSED_CRPS=0 computes the term from torch
# ops on the same member states (ops.crps_ens_torch: the rollout's launches stay, only the term is swapped) for A/B runs and tests
FUSED_CRPS = _os.environ.get("NLAM_FUSED_CRPS", "1") == "1"
# output clamping and the predicted std inside the step-tail pass (ops.StepTailExtFunction); NLAM_FUSED_CLAMPED_TAIL=0 restores the
# torch-op tail of such models (get_clamped_new_state, softplus, the loss pass over the rollout) for A/B runs.  On: at cfg2 size
# 1.75 against 1.80 ms per step with a predicted std, 1.72 against 2.71 ms with three clamps (profiles/clamped_tail/README.md)
FUSED_CLAMPED_TAIL = _os.environ.get("NLAM_FUSED_CLAMPED_TAIL", "1") == "1"
# static-feature embedders (keys of static_embedding_specs: "mesh", "g2m", "m2g", "m2m", ..; "all") whose backward runs as soon as
# the gradient of their output is complete instead of in the grouped launch at the very end of backward (NLAM_EARLY_EMB; default none)
EARLY_EMBEDDER_BACKWARD = frozenset(k for k in _os.environ.get("NLAM_EARLY_EMB", "").split(",") if k)

class BufferList(nn.Module):
    """utils/buffer_list.py:11: list of non-persistent buffers."""

    def __init__(self, tensors, persistent=False):
        super().__init__()
        self.n_buffers = len(tensors)
        for i, t in enumerate(tensors):
            self.register_buffer(f"b{i}", t, persistent=persistent)

    def __getitem__(self, k):
        if isinstance(k, slice):
            return [self[i] for i in range(*k.indices(self.n_buffers))]
        if k < 0:
            k += self.n_buffers
        if not 0 <= k < self.n_buffers:
            raise IndexError(f"index {k} out of range for BufferList of length {self.n_buffers}")
        return getattr(self, f"b{k}")

    def __len__(self):
        return self.n_buffers

    def __iter__(self):
        return (self[i] for i in range(self.n_buffers))


def _rebuild_clamp_tables(module, incompatible_keys):
    """load_state_dict post hook of a StepPredictor (a module-level function: the module stays picklable)."""
    module.clamp_tables()


class StepPredictor(nn.Module):
    def __init__(self, datastore, output_std=False, output_clamping_lower=None, output_clamping_upper=None):
        super().__init__()
        self._output_clamping_lower = dict(output_clamping_lower) if output_clamping_lower else {}
        self._output_clamping_upper = dict(output_clamping_upper) if output_clamping_upper else {}
        num_state_vars = datastore.get_num_data_vars(category="state")
        da_static = datastore.get_dataarray(category="static", split=None, standardize=True)
        if da_static is None:
            static = torch.empty((datastore.num_grid_points, 0), dtype=torch.float32)
        else:
            static = torch.tensor(da_static.values, dtype=torch.float32)
        self.register_buffer("grid_static_features", static, persistent=False)
        st = datastore.get_standardization_dataarray(category="state")
        self.register_buffer("state_mean", torch.tensor(st.state_mean.values, dtype=torch.float32), persistent=False)
        self.register_buffer("state_std", torch.tensor(st.state_std.values, dtype=torch.float32), persistent=False)
        self.output_std = bool(output_std)
        self.grid_output_dim = 2 * num_state_vars if self.output_std else num_state_vars
        self.num_grid_nodes = self.grid_static_features.shape[0]

    @property
    def predicts_std(self) -> bool:
        return self.output_std

    def expand_to_batch(self, x, batch_size):
        return x.unsqueeze(0).expand(batch_size, -1, -1)

    def prepare_clamping_params(self, datastore):
        names = datastore.get_vars_names(category="state")
        lower, upper = self._output_clamping_lower, self._output_clamping_upper
        unknown = (set(lower) - set(names)) | (set(upper) - set(names))
        if unknown:
            raise ValueError(f"State feature limits were provided for unknown features: {unknown}")

        def norm(x, i):
            return (x - self.state_mean[i]) / self.state_std[i]

        lu_idx, lu_lo, lu_hi, lo_idx, lo_lim, hi_idx, hi_lim = [], [], [], [], [], [], []
        for i, f in enumerate(names):
            if f in lower and f in upper:
                assert lower[f] < upper[f], f'Invalid clamping limits for feature "{f}"'
                lu_idx.append(i)
                lu_lo.append(norm(lower[f], i))
                lu_hi.append(norm(upper[f], i))
            elif f in lower:
                lo_idx.append(i)
                lo_lim.append(norm(lower[f], i))
            elif f in upper:
                hi_idx.append(i)
                hi_lim.append(norm(upper[f], i))
        self.register_buffer("sigmoid_lower_lims", torch.tensor(lu_lo))
        self.register_buffer("sigmoid_upper_lims", torch.tensor(lu_hi))
        self.register_buffer("softplus_lower_lims", torch.tensor(lo_lim))
        self.register_buffer("softplus_upper_lims", torch.tensor(hi_lim))
        self.register_buffer("clamp_lower_upper_idx", torch.tensor(lu_idx))
        self.register_buffer("clamp_lower_idx", torch.tensor(lo_idx))
        self.register_buffer("clamp_upper_idx", torch.tensor(hi_idx))
        # the kernel's tables follow the buffers: built here, after every .to() / .float() (_apply) and after load_state_dict, so that
        # no call inside a stream capture has to build them (the first build copies the index buffers to the host)
        self.clamp_tables()
        self.register_load_state_dict_post_hook(_rebuild_clamp_tables)

    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        if hasattr(self, "clamp_upper_idx"):
            self.clamp_tables()
        return out

    def __setstate__(self, state):
        # copy.deepcopy / unpickling: the copied tables are keyed on the original's buffers, so build this module's own here
        super().__setstate__(state)
        self.__dict__.pop("_clamp_tables", None)
        if hasattr(self, "clamp_upper_idx"):
            self.clamp_tables()

    def clamp_tables(self):
        """The clamps as one per-variable table (ops.ClampTables: mode NLAM_CLAMP_* on the host, lo / hi standardised limits
        where the model lives, 0 where a variable has no such limit), None for a model without clamps.  Built from the buffers
        prepare_clamping_params registers, there and whenever they are replaced or written (``_apply``, ``load_state_dict``); the
        key below only catches a buffer written by hand, and rebuilding then synchronises with the device."""
        from ._lib import CLAMP_BOTH, CLAMP_LOWER, CLAMP_UPPER
        from .ops import ClampTables

        bufs = (self.clamp_lower_upper_idx, self.clamp_lower_idx, self.clamp_upper_idx, self.sigmoid_lower_lims,
                self.sigmoid_upper_lims, self.softplus_lower_lims, self.softplus_upper_lims)
        if sum(b.numel() for b in bufs[:3]) == 0:
            return None
        key = tuple((id(b), b._version) for b in bufs)
        cached = getattr(self, "_clamp_tables", None)
        if cached is not None and cached[0] == key:
            return cached[1]
        lu, lo_i, hi_i = (b.long() for b in bufs[:3])
        n = self.state_mean.shape[0]
        modes = torch.zeros(n, dtype=torch.int32)
        lo = torch.zeros(n, dtype=torch.float32, device=self.state_mean.device)
        hi = torch.zeros_like(lo)
        modes[lu.cpu()], modes[lo_i.cpu()], modes[hi_i.cpu()] = CLAMP_BOTH, CLAMP_LOWER, CLAMP_UPPER
        lo[lu], hi[lu] = bufs[3].float(), bufs[4].float()
        lo[lo_i] = bufs[5].float()
        hi[hi_i] = bufs[6].float()
        tables = ClampTables(modes.tolist(), lo, hi)
        self._clamp_tables = (key, tables)
        return tables

    def get_clamped_new_state(self, state_delta, prev_state):
        sp = torch.nn.functional.softplus
        new_state = prev_state + state_delta
        if self.clamp_lower_upper_idx.numel() > 0:
            idx = self.clamp_lower_upper_idx
            lo, hi = self.sigmoid_lower_lims, self.sigmoid_upper_lims
            inv = inverse_sigmoid((prev_state[:, :, idx] - lo) / (hi - lo))
            new_state[:, :, idx] = lo + (hi - lo) * torch.sigmoid(inv + state_delta[:, :, idx])
        if self.clamp_lower_idx.numel() > 0:
            idx = self.clamp_lower_idx
            lo = self.softplus_lower_lims
            inv = inverse_softplus(prev_state[:, :, idx] - lo, beta=1)
            new_state[:, :, idx] = lo + sp(inv + state_delta[:, :, idx], beta=1)
        if self.clamp_upper_idx.numel() > 0:
            idx = self.clamp_upper_idx
            hi = self.softplus_upper_lims
            inv = -inverse_softplus(hi - prev_state[:, :, idx], beta=1)
            new_state[:, :, idx] = hi - sp(-(inv + state_delta[:, :, idx]), beta=1)
        return new_state


def compute_grid_input_dim(datastore, num_past_forcing_steps, num_future_forcing_steps):
    """utils/graph.py:470-512."""
    n_state = datastore.get_num_data_vars(category="state")
    n_forcing = datastore.get_num_data_vars(category="forcing")
    da_static = datastore.get_dataarray(category="static", split=None)
    n_static = 0 if da_static is None else datastore.get_num_data_vars(category="static")
    return 2 * n_state + n_static + n_forcing * (num_past_forcing_steps + num_future_forcing_steps + 1)


class BaseGraphModel(StepPredictor):
    def __init__(
        self,
        datastore,
        graph_name: str = "multiscale",
        hidden_dim: int = 64,
        hidden_layers: int = 1,
        processor_layers: int = 4,
        mesh_aggr: str = "sum",
        num_past_forcing_steps: int = 1,
        num_future_forcing_steps: int = 1,
        output_std: bool = False,
        output_clamping_lower=None,
        output_clamping_upper=None,
        g2m_gnn_type: str = "InteractionNet",
        m2g_gnn_type: str = "InteractionNet",
        graph=None,
    ):
        super().__init__(datastore, output_std, output_clamping_lower, output_clamping_upper)
        self.g2m_gnn_type, self.m2g_gnn_type = g2m_gnn_type, m2g_gnn_type
        st = datastore.get_standardization_dataarray("state")
        self.register_buffer(
            "diff_mean", torch.tensor(st.state_diff_mean_standardized.values, dtype=torch.float32), persistent=False
        )
        self.register_buffer(
            "diff_std", torch.tensor(st.state_diff_std_standardized.values, dtype=torch.float32), persistent=False
        )
        self.hidden_dim, self.hidden_layers = hidden_dim, hidden_layers
        self.processor_layers, self.mesh_aggr = processor_layers, mesh_aggr
        if graph is None:
            ext = datastore.get_xy_extent(category="state")
            span = max(ext[1] - ext[0], ext[3] - ext[2])  # graph/base.py:113-117
            graph = G.load_graph(datastore.root_path / "graph" / graph_name, span)
        self.hierarchical, tensors = graph
        for name, value in tensors.items():  # utils/graph.py:461-466: non-persistent buffers
            if torch.is_tensor(value):
                self.register_buffer(name, value.clone(), persistent=False)
            else:
                setattr(self, name, BufferList([v.clone() for v in value], persistent=False))
        self.num_mesh_nodes, _ = self.get_num_mesh()
        self.grid_input_dim = compute_grid_input_dim(datastore, num_past_forcing_steps, num_future_forcing_steps)
        self.g2m_edges, g2m_dim = self.g2m_features.shape
        self.m2g_edges, m2g_dim = self.m2g_features.shape
        self.mlp_blueprint_end = [hidden_dim] * (hidden_layers + 1)
        self.grid_embedder = make_mlp([self.grid_input_dim] + self.mlp_blueprint_end)
        self.g2m_embedder = make_mlp([g2m_dim] + self.mlp_blueprint_end)
        self.m2g_embedder = make_mlp([m2g_dim] + self.mlp_blueprint_end)
        self.g2m_gnn = get_gnn_class(g2m_gnn_type)(
            self.g2m_edge_index, hidden_dim, hidden_layers=hidden_layers, update_edges=False
        )
        self.encoding_grid_mlp = make_mlp([hidden_dim] + self.mlp_blueprint_end)
        self.m2g_gnn = get_gnn_class(m2g_gnn_type)(
            self.m2g_edge_index, hidden_dim, hidden_layers=hidden_layers, update_edges=False
        )
        self.output_map = make_mlp([hidden_dim] * (hidden_layers + 1) + [self.grid_output_dim], layer_norm=False)
        self.prepare_clamping_params(datastore)
        self._static = None  # cache of input-independent embeddings during a rollout
        from .ops import MlpGeometry
        from . import _lib as L

        self._enc_geom = MlpGeometry(nsrc=1, flags=L.F_ADD_SRC0)  # grid_emb + encoding_grid_mlp(grid_emb)

    # ---- input-independent embeddings: once per rollout instead of once per AR step ----
    def static_embedding_items(self):
        """(key, thunk) in the order the step needs them (encoder first, decoder last)."""
        return [
            ("mesh", self.embedd_mesh_nodes),
            ("g2m", lambda: self.g2m_embedder(self.g2m_features)),
            ("m2g", lambda: self.m2g_embedder(self.m2g_features)),
        ]

    def static_embedding_specs(self):
        """(key, mlp | [mlps], features | [features]) in the order the step needs them: the embedders of the static
        features are independent of each other and of the input, so they run as grouped launches."""
        return [
            ("mesh", *self.mesh_embedding_spec()),
            ("g2m", self.g2m_embedder, self.g2m_features),
            ("m2g", self.m2g_embedder, self.m2g_features),
        ]

    def compute_static_embeddings(self) -> dict:
        from .gnn_layers import grouped_mlp_forward

        specs = self.static_embedding_specs()
        pairs, slots = [], []
        for key, mlps, feats in specs:
            if isinstance(mlps, (list, tuple, nn.ModuleList)):
                for i, (m_, f_) in enumerate(zip(mlps, feats)):
                    pairs.append((m_, f_))
                    slots.append((key, i))
            else:
                pairs.append((mlps, feats))
                slots.append((key, None))
        from . import ops

        outs = grouped_mlp_forward(pairs)
        # embedders whose output gradient is complete long before the end of backward run their backward right then, on a side
        # stream (ops.early_backward_leaf).  Measured (round 6, profiles/round6/ab_early_emb.log): the mesh -> grid edge embedder
        # (64 % of the grouped backward's rows at MEPS size; its gradient is final behind the decoder's backward) leaves the tail of
        # the cfg2 step -- and the step does not move (1.7564 vs 1.7565 ms; cfg3 / cfg4 within noise): the chip is time-shared
        # either way.  Off by default (NLAM_EARLY_EMB=m2g, or "all", switches it on)
        early = EARLY_EMBEDDER_BACKWARD
        outs = [ops.early_backward_leaf(o, force=True) if (key in early or "all" in early) and o.requires_grad else o
                for (key, _i), o in zip(slots, outs)]
        st = {}
        for (key, i), o in zip(slots, outs):
            if i is None:
                st[key] = o
            else:
                st.setdefault(key, []).append(o)
        # the embeddings live for a whole rollout: their consumers' backward passes hand the gradient over in one buffer
        ops.rollout_shared_reset(outs)
        for key, mlps, _ in specs:   # empty lists (a one-level hierarchy has no up / down embedders)
            if isinstance(mlps, (list, tuple, nn.ModuleList)) and key not in st:
                st[key] = []
        return st

    @contextlib.contextmanager
    def static_cache(self):
        """Embeddings of the static graph features, computed once for a whole rollout.  (Computing them on side
        streams next to the first grid MLPs was measured and dropped: -1 % with one side stream, -3 % with one per
        embedder -- DESIGN.md, "measured and dropped".)"""
        self._static = self.compute_static_embeddings()
        try:
            yield
        finally:
            self._static = None

    def can_return_raw_delta(self) -> bool:
        """True when the step's tail is the plain ``prev + delta * diff_std + diff_mean`` (no clamping, no predicted std):
        the forecaster may then fuse it with the boundary overwrite and the loss (ops.StepTailFunction)."""
        no_clamp = self.clamp_lower_upper_idx.numel() + self.clamp_lower_idx.numel() + self.clamp_upper_idx.numel() == 0
        return no_clamp and not self.output_std and self.diff_std.dim() == 1

    def can_fuse_ext_tail(self) -> bool:
        """True when the step's tail has output clamps and / or a predicted std and may run as one pass with the boundary
        overwrite and the loss term (ops.StepTailExtFunction on the raw network output); FUSED_CLAMPED_TAIL = False says no."""
        no_clamp = self.clamp_lower_upper_idx.numel() + self.clamp_lower_idx.numel() + self.clamp_upper_idx.numel() == 0
        return FUSED_CLAMPED_TAIL and (self.output_std or not no_clamp) and self.diff_std.dim() == 1

    def forward(self, prev_state, prev_prev_state, forcing, raw_delta: bool = False):
        B = prev_state.shape[0]
        feats = (prev_state, prev_prev_state, forcing, self.expand_to_batch(self.grid_static_features, B))
        st = self._static if self._static is not None else self.compute_static_embeddings()
        fused_ok = FUSED_STATE_UPDATE and prev_state.is_cuda and all(t.dtype == torch.float32 and t.dim() == 3 for t in feats)
        if fused_ok and FOLD_INPUT_CAT and self.grid_embedder.fully_fused and self.grid_input_dim <= 64 and self.grid_input_dim % 4 == 0:
            from .ops import CatMLPFunction

            # graph/base.py:275-286: the torch.cat of the input features folded into grid_embedder's first load (the (B, N, 56)
            # tensor is only written as a by-product for the backward pass; the static features are read un-expanded)
            grid_emb = CatMLPFunction.apply(*self.grid_embedder.params(), *feats)
        else:
            if fused_ok:
                from .ops import ConcatFunction

                grid_features = ConcatFunction.apply(*feats)   # graph/base.py:275-283 in one launch; the static features are read un-expanded
            else:
                grid_features = torch.cat(feats, dim=-1)
            grid_emb = self.grid_embedder(grid_features)  # (B, N_grid, d)
        mesh_rep = self.g2m_gnn(
            grid_emb, self.expand_to_batch(st["mesh"], B), self.expand_to_batch(st["g2m"], B)
        )
        # graph/base.py:308.  Kept after the g2m step as in the reference: issuing it first (it is independent) measured
        # 2 % slower at cfg2 -- its 16 MB output then sits cold through the whole processor before m2g reads it.
        if self.encoding_grid_mlp.fully_fused:
            grid_rep, _ = self.encoding_grid_mlp.forward_fused(self._enc_geom, grid_emb)
        else:
            grid_rep = grid_emb + self.encoding_grid_mlp(grid_emb)
        mesh_rep = self.process_step(mesh_rep, st)
        grid_rep = self.m2g_gnn(mesh_rep, grid_rep, self.expand_to_batch(st["m2g"], B))
        net_output = self.output_map(grid_rep)
        if raw_delta:
            return net_output, None
        if self.output_std:
            pred_delta_mean, pred_std_raw = net_output.chunk(2, dim=-1)
            pred_std = torch.nn.functional.softplus(pred_std_raw)
        else:
            pred_delta_mean, pred_std = net_output, None
        no_clamp = self.clamp_lower_upper_idx.numel() + self.clamp_lower_idx.numel() + self.clamp_upper_idx.numel() == 0
        if (FUSED_STATE_UPDATE and no_clamp and pred_delta_mean.is_cuda and self.diff_std.dim() == 1
                and pred_delta_mean.dtype == torch.float32 and prev_state.dtype == torch.float32):
            from .ops import AffineMixFunction

            # prev_state + (delta * diff_std + diff_mean) in one pass (three elementwise launches in the reference)
            new_state = AffineMixFunction.apply(None, None, prev_state, None, pred_delta_mean, self.diff_std, self.diff_mean)
            return new_state, pred_std
        rescaled = pred_delta_mean * self.diff_std + self.diff_mean
        return self.get_clamped_new_state(rescaled, prev_state), pred_std


class GraphLAM(BaseGraphModel):
    def __init__(self, datastore, graph_name="multiscale", **kw):
        super().__init__(datastore, graph_name, **kw)
        assert not self.hierarchical, "GraphLAM does not use a hierarchical mesh graph"
        mesh_dim = self.mesh_static_features.shape[1]
        _, m2m_dim = self.m2m_features.shape
        self.mesh_embedder = make_mlp([mesh_dim] + self.mlp_blueprint_end)
        self.m2m_embedder = make_mlp([m2m_dim] + self.mlp_blueprint_end)
        self.processor = GNNSequential(
            [
                InteractionNet(
                    self.m2m_edge_index, self.hidden_dim, hidden_layers=self.hidden_layers, aggr=self.mesh_aggr
                )
                for _ in range(self.processor_layers)
            ]
        )

    def get_num_mesh(self):
        return self.mesh_static_features.shape[0], 0

    def embedd_mesh_nodes(self):
        return self.mesh_embedder(self.mesh_static_features)

    def mesh_embedding_spec(self):
        return self.mesh_embedder, self.mesh_static_features

    def static_embedding_items(self):
        items = super().static_embedding_items()
        return items[:2] + [("m2m", lambda: self.m2m_embedder(self.m2m_features))] + items[2:]

    def static_embedding_specs(self):
        specs = super().static_embedding_specs()
        return specs[:2] + [("m2m", self.m2m_embedder, self.m2m_features)] + specs[2:]

    def process_step(self, mesh_rep, st=None):
        B = mesh_rep.shape[0]
        m2m_emb = st["m2m"] if st is not None else self.m2m_embedder(self.m2m_features)
        mesh_rep, _ = self.processor(mesh_rep, self.expand_to_batch(m2m_emb, B), need_last_edges=False)
        return mesh_rep


class BaseHiGraphModel(BaseGraphModel):
    def __init__(
        self, datastore, graph_name="multiscale", mesh_up_gnn_type="InteractionNet",
        mesh_down_gnn_type="InteractionNet", **kw,
    ):
        super().__init__(datastore, graph_name, **kw)
        self.mesh_up_gnn_type, self.mesh_down_gnn_type = mesh_up_gnn_type, mesh_down_gnn_type
        self.num_levels = len(self.mesh_static_features)
        self.level_mesh_sizes = [m.shape[0] for m in self.mesh_static_features]
        mesh_dim = self.mesh_static_features[0].shape[1]
        same_dim = self.m2m_features[0].shape[1]
        up_dim = self.mesh_up_features[0].shape[1]
        down_dim = self.mesh_down_features[0].shape[1]
        end, L_ = self.mlp_blueprint_end, self.num_levels
        self.mesh_embedders = nn.ModuleList([make_mlp([mesh_dim] + end) for _ in range(L_)])
        self.mesh_same_embedders = nn.ModuleList([make_mlp([same_dim] + end) for _ in range(L_)])
        self.mesh_up_embedders = nn.ModuleList([make_mlp([up_dim] + end) for _ in range(L_ - 1)])
        self.mesh_down_embedders = nn.ModuleList([make_mlp([down_dim] + end) for _ in range(L_ - 1)])
        up_cls, down_cls = get_gnn_class(mesh_up_gnn_type), get_gnn_class(mesh_down_gnn_type)
        self.mesh_init_gnns = nn.ModuleList(
            [up_cls(ei, self.hidden_dim, hidden_layers=self.hidden_layers) for ei in self.mesh_up_edge_index]
        )
        self.mesh_read_gnns = nn.ModuleList(
            [
                down_cls(ei, self.hidden_dim, hidden_layers=self.hidden_layers, update_edges=False)
                for ei in self.mesh_down_edge_index
            ]
        )

    def get_num_mesh(self):
        n = sum(m.shape[0] for m in self.mesh_static_features)
        return n, n - self.mesh_static_features[0].shape[0]

    def embedd_mesh_nodes(self):
        return self.mesh_embedders[0](self.mesh_static_features[0])

    def mesh_embedding_spec(self):
        return self.mesh_embedders[0], self.mesh_static_features[0]

    def static_embedding_specs(self):
        specs = super().static_embedding_specs()
        mine = [
            ("levels", list(self.mesh_embedders)[1:], list(self.mesh_static_features[1:])),
            ("up", list(self.mesh_up_embedders), list(self.mesh_up_features)),
            ("same", list(self.mesh_same_embedders), list(self.m2m_features)),
            ("down", list(self.mesh_down_embedders), list(self.mesh_down_features)),
        ]
        return specs[:2] + mine + specs[2:]

    def static_embedding_items(self):
        items = super().static_embedding_items()
        mine = [
            ("levels", lambda: [emb(f) for emb, f in zip(list(self.mesh_embedders)[1:], self.mesh_static_features[1:])]),
            ("up", lambda: [emb(f) for emb, f in zip(self.mesh_up_embedders, self.mesh_up_features)]),
            ("same", lambda: [emb(f) for emb, f in zip(self.mesh_same_embedders, self.m2m_features)]),
            ("down", lambda: [emb(f) for emb, f in zip(self.mesh_down_embedders, self.mesh_down_features)]),
        ]
        return items[:2] + mine + items[2:]

    def process_step(self, mesh_rep, st=None):
        B = mesh_rep.shape[0]
        if st is None:
            st = self.compute_static_embeddings()
        ex = self.expand_to_batch
        levels = [mesh_rep] + [ex(e, B) for e in st["levels"]]
        same = [ex(e, B) for e in st["same"]]
        up = [ex(e, B) for e in st["up"]]
        down = [ex(e, B) for e in st["down"]]
        for l, gnn in enumerate(self.mesh_init_gnns, start=1):  # hierarchical.py:241-262
            levels[l], up[l - 1] = gnn(levels[l - 1], levels[l], up[l - 1])
        levels, _, _, down = self.hi_processor_step(levels, same, up, down)
        for l, gnn in zip(range(self.num_levels - 2, -1, -1), reversed(self.mesh_read_gnns)):  # :271-289
            levels[l] = gnn(levels[l + 1], levels[l], down[l])
        return levels[0]


class HiLAM(BaseHiGraphModel):
    def __init__(self, datastore, graph_name="multiscale", **kw):
        super().__init__(datastore, graph_name, **kw)
        P = self.processor_layers
        self.mesh_down_gnns = nn.ModuleList([self.make_down_gnns() for _ in range(P)])
        self.mesh_down_same_gnns = nn.ModuleList([self.make_same_gnns() for _ in range(P)])
        self.mesh_up_gnns = nn.ModuleList([self.make_up_gnns() for _ in range(P)])
        self.mesh_up_same_gnns = nn.ModuleList([self.make_same_gnns() for _ in range(P)])

    def make_same_gnns(self):
        return nn.ModuleList(
            [InteractionNet(ei, self.hidden_dim, hidden_layers=self.hidden_layers) for ei in self.m2m_edge_index]
        )

    def make_up_gnns(self):
        cls = get_gnn_class(self.mesh_up_gnn_type)
        return nn.ModuleList([cls(ei, self.hidden_dim, hidden_layers=self.hidden_layers) for ei in self.mesh_up_edge_index])

    def make_down_gnns(self):
        cls = get_gnn_class(self.mesh_down_gnn_type)
        return nn.ModuleList(
            [cls(ei, self.hidden_dim, hidden_layers=self.hidden_layers) for ei in self.mesh_down_edge_index]
        )

    def mesh_down_step(self, levels, same, down, down_gnns, same_gnns):  # hi_lam.py:167-236
        levels[-1], same[-1] = same_gnns[-1](levels[-1], levels[-1], same[-1])
        for l, dg, sg in zip(range(self.num_levels - 2, -1, -1), reversed(down_gnns), reversed(same_gnns[:-1])):
            new_node, down[l] = dg(levels[l + 1], levels[l], down[l])
            levels[l], same[l] = sg(new_node, new_node, same[l])
        return levels, same, down

    def mesh_up_step(self, levels, same, up, up_gnns, same_gnns):  # hi_lam.py:238-307
        levels[0], same[0] = same_gnns[0](levels[0], levels[0], same[0])
        for l, (ug, sg) in enumerate(zip(up_gnns, same_gnns[1:]), start=1):
            new_node, up[l - 1] = ug(levels[l - 1], levels[l], up[l - 1])
            levels[l], same[l] = sg(new_node, new_node, same[l])
        return levels, same, up

    def hi_processor_step(self, levels, same, up, down):  # hi_lam.py:309-376
        for dg, dsg, ug, usg in zip(
            self.mesh_down_gnns, self.mesh_down_same_gnns, self.mesh_up_gnns, self.mesh_up_same_gnns
        ):
            levels, same, down = self.mesh_down_step(levels, same, down, dg, dsg)
            levels, same, up = self.mesh_up_step(levels, same, up, ug, usg)
        return levels, same, up, down


class HiLAMParallel(BaseHiGraphModel):
    def __init__(self, datastore, graph_name="multiscale", **kw):
        super().__init__(datastore, graph_name, **kw)
        first = [0]
        for size in self.level_mesh_sizes[:-1]:
            first.append(first[-1] + size)
        off_m2m = [ei + o for ei, o in zip(self.m2m_edge_index, first)]
        off_up = [
            torch.stack((ei[0] + first[l], ei[1] + first[l + 1]), dim=0) for l, ei in enumerate(self.mesh_up_edge_index)
        ]
        off_down = [
            torch.stack((ei[0] + first[l + 1], ei[1] + first[l]), dim=0)
            for l, ei in enumerate(self.mesh_down_edge_index)
        ]
        total_list = off_m2m + off_up + off_down
        total = torch.cat(total_list, dim=1)
        self.edge_split_sections = [ei.shape[1] for ei in total_list]
        if self.processor_layers == 0:
            self.processor = lambda x, edge_attr: (x, edge_attr)
        else:
            self.processor = GNNSequential(
                [
                    InteractionNet(
                        total,
                        self.hidden_dim,
                        hidden_layers=self.hidden_layers,
                        edge_chunk_sizes=self.edge_split_sections,
                        aggr_chunk_sizes=self.level_mesh_sizes,
                    )
                    for _ in range(self.processor_layers)
                ]
            )

    def hi_processor_step(self, levels, same, up, down):  # hi_lam_parallel.py:145-218
        mesh_rep = torch.cat(levels, dim=1)
        edge_rep = torch.cat(same + up + down, dim=1)
        mesh_rep, edge_rep = self.processor(mesh_rep, edge_rep)
        levels = list(torch.split(mesh_rep, self.level_mesh_sizes, dim=1))
        sec = torch.split(edge_rep, self.edge_split_sections, dim=1)
        L_ = self.num_levels
        return levels, list(sec[:L_]), list(sec[L_ : L_ + (L_ - 1)]), list(sec[L_ + (L_ - 1) :])


MODELS = {"graph_lam": GraphLAM, "hi_lam": HiLAM, "hi_lam_parallel": HiLAMParallel}  # models/__init__.py:23-27


class ARForecaster(nn.Module):
    """models/forecasters/autoregressive.py:14-149."""

    def __init__(self, predictor, datastore):
        super().__init__()
        self.predictor = predictor
        bm = torch.tensor(datastore.boundary_mask.values, dtype=torch.float32).unsqueeze(0).unsqueeze(-1)
        self.register_buffer("boundary_mask", bm, persistent=False)
        self.register_buffer("interior_mask", 1.0 - self.boundary_mask, persistent=False)

    @property
    def predicts_std(self):
        return self.predictor.predicts_std

    def takes_ext_tail(self, init_states, boundary_states) -> bool:
        """Whether ``forward`` runs the tail of these inputs on ops.StepTailExtFunction: a predictor with output clamps or a
        predicted std (``can_fuse_ext_tail``, never true together with ``can_return_raw_delta``), fp32 tensors on the GPU."""
        return (FUSED_STATE_UPDATE and init_states.is_cuda and init_states.dtype == torch.float32
                and boundary_states.dtype == torch.float32 and getattr(self.predictor, "can_fuse_ext_tail", lambda: False)())

    def forward(self, init_states, forcing_features, boundary_states, loss_spec=None):
        """``loss_spec = (target_states, inv_var (F,), row_weight (N,), scale)``: also return the training loss
        ``scale * sum_t sum_n,f row_weight * inv_var * (pred - target)^2`` as a third value, with each step's state
        update + boundary overwrite + loss term fused into one pass (ops.StepTailFunction) when the predictor's tail is
        the plain rescale (no clamping / predicted std).  ``loss_spec = (target_states, var_std (F,), row_weight (N,), scale,
        kind)`` with a ``_lib.LOSS_*`` kind: the same for that loss with the per-variable std ``var_std`` (the same
        Function, ``kind`` given); the third value is None where the tail cannot be fused.  A predictor with output
        clamps or a predicted std (``can_fuse_ext_tail``) takes ops.StepTailExtFunction instead, with or without a ``loss_spec``: the
        five-entry spec gives its loss term (``var_std`` None with a predicted std); the four-entry one is wmse, so it runs as
        ``NLAM_LOSS_WMSE`` on the predicted std, or on ``var_std = inv_var ** -0.5`` (one small launch per call: hand in the std)."""
        prev_prev_state, prev_state = init_states[:, 0], init_states[:, 1]
        preds, stds = [], []
        cache = self.predictor.static_cache() if hasattr(self.predictor, "static_cache") else contextlib.nullcontext()
        fused_tail = (loss_spec is not None and FUSED_STATE_UPDATE and init_states.is_cuda and init_states.dtype == torch.float32
                      and boundary_states.dtype == torch.float32 and getattr(self.predictor, "can_return_raw_delta", lambda: False)()
                      and not getattr(self.predictor, "draws_latent", False))   # Graph-EFM keeps its own tail in a rollout
        ext_tail = self.takes_ext_tail(init_states, boundary_states)
        losses = []
        if ext_tail and loss_spec is not None:
            ext_spec = loss_spec
            if len(loss_spec) == 4:   # the wmse form: the kind's entry takes a std
                from ._lib import LOSS_WMSE

                target, inv_var, row_weight, scale = loss_spec
                ext_spec = (target, None if self.predictor.output_std else torch.rsqrt(inv_var), row_weight, scale, LOSS_WMSE)
        with cache:
            for i in range(forcing_features.shape[1]):
                if ext_tail:
                    from .ops import StepTailExtFunction

                    delta, _ = self.predictor(prev_state, prev_prev_state, forcing_features[:, i], raw_delta=True)
                    target_i = consts = row_weight = kind = None
                    scale = 1.0
                    if loss_spec is not None:
                        target, consts, row_weight, scale, kind = ext_spec
                        target_i = target[:, i]
                    new_state, pred_std, loss_t = StepTailExtFunction.apply(
                        delta.float(), prev_state, boundary_states[:, i], target_i, self.predictor.diff_std, self.predictor.diff_mean,
                        self.boundary_mask.reshape(-1), consts, row_weight, scale, kind, self.predictor.clamp_tables())
                    preds.append(new_state)
                    if pred_std is not None:
                        stds.append(pred_std)
                    if loss_t is not None:
                        losses.append(loss_t)
                    prev_prev_state, prev_state = prev_state, new_state
                    continue
                if fused_tail:
                    from .ops import StepTailFunction

                    delta, _ = self.predictor(prev_state, prev_prev_state, forcing_features[:, i], raw_delta=True)
                    target, consts, row_weight, scale, kind = loss_spec if len(loss_spec) == 5 else (*loss_spec, None)
                    new_state, loss_t = StepTailFunction.apply(
                        delta.float(), prev_state, boundary_states[:, i], target[:, i], self.predictor.diff_std,
                        self.predictor.diff_mean, self.boundary_mask.reshape(-1), consts, row_weight, scale, kind)
                    preds.append(new_state)
                    losses.append(loss_t)
                    prev_prev_state, prev_state = prev_state, new_state
                    continue
                pred_state, pred_std = self.predictor(prev_state, prev_prev_state, forcing_features[:, i])
                if (FUSED_STATE_UPDATE and pred_state.is_cuda and pred_state.dtype == torch.float32
                        and boundary_states.dtype == torch.float32):
                    from .ops import AffineMixFunction

                    # autoregressive.py:128-131 in one pass
                    new_state = AffineMixFunction.apply(boundary_states[:, i], self.boundary_mask.reshape(-1), pred_state,
                                                        self.interior_mask.reshape(-1), None, None, None)
                else:
                    new_state = self.boundary_mask * boundary_states[:, i] + self.interior_mask * pred_state
                preds.append(new_state)
                if pred_std is not None:
                    stds.append(pred_std)
                prev_prev_state, prev_state = prev_state, new_state
        def _stack(xs):   # a one-step rollout needs no copy
            return xs[0].unsqueeze(1) if len(xs) == 1 else torch.stack(xs, dim=1)

        if loss_spec is not None:
            loss = None
            if losses:
                loss = losses[0] if len(losses) == 1 else torch.stack(losses).sum()
            return _stack(preds), (_stack(stds) if stds else None), loss
        return _stack(preds), (_stack(stds) if stds else None)


def mask_and_reduce_metric(vals, mask, average_grid, sum_vars):
    """metrics.py:37-84.  ``mask`` may be the reference's boolean node mask or a precomputed
    int64 index of the selected nodes (same entries in the same order, but a static gather:
    no nonzero() -> no host synchronisation, so the step can live in a HIP graph)."""
    if mask is not None:
        vals = vals[..., mask, :] if mask.dtype == torch.bool else vals.index_select(-2, mask)
    if average_grid:
        vals = torch.mean(vals, dim=-2)
    if sum_vars:
        vals = torch.sum(vals, dim=-1)
    return vals


def wmse(pred, target, pred_std, mask=None, average_grid=True, sum_vars=True):
    """metrics.py:87-137."""
    entry = torch.nn.functional.mse_loss(pred, target, reduction="none") / (pred_std**2)
    return mask_and_reduce_metric(entry, mask, average_grid, sum_vars)


# The other metrics of metrics.DEFINED_METRICS as plain torch formulas, for evaluation code; training runs them on
# ops.LossFunction / ops.StepTailFunction (ForecasterStep(loss=...)).
def mse(pred, target, pred_std, mask=None, average_grid=True, sum_vars=True):
    """metrics.py:140-182: wmse with the std replaced by ones."""
    return wmse(pred, target, torch.ones_like(pred_std), mask, average_grid, sum_vars)


def wmae(pred, target, pred_std, mask=None, average_grid=True, sum_vars=True):
    """metrics.py:185-235."""
    entry = torch.nn.functional.l1_loss(pred, target, reduction="none") / pred_std
    return mask_and_reduce_metric(entry, mask, average_grid, sum_vars)


def mae(pred, target, pred_std, mask=None, average_grid=True, sum_vars=True):
    """metrics.py:238-280: wmae with the std replaced by ones."""
    return wmae(pred, target, torch.ones_like(pred_std), mask, average_grid, sum_vars)


def nll(pred, target, pred_std, mask=None, average_grid=True, sum_vars=True):
    """metrics.py:283-329: -log N(target; pred, pred_std)."""
    entry = -torch.distributions.Normal(pred, pred_std).log_prob(target)
    return mask_and_reduce_metric(entry, mask, average_grid, sum_vars)


def crps_gauss(pred, target, pred_std, mask=None, average_grid=True, sum_vars=True):
    """metrics.py:332-386: closed-form CRPS of a Gaussian."""
    std_normal = torch.distributions.Normal(torch.zeros((), device=pred.device), torch.ones((), device=pred.device))
    z = (target - pred) / pred_std
    entry = -pred_std * (torch.pi ** (-0.5) - 2 * torch.exp(std_normal.log_prob(z)) - z * (2 * std_normal.cdf(z) - 1))
    return mask_and_reduce_metric(entry, mask, average_grid, sum_vars)


DEFINED_METRICS = {"mse": mse, "mae": mae, "wmse": wmse, "wmae": wmae, "nll": nll, "crps_gauss": crps_gauss}


def get_metric(metric_name):
    """metrics.py:10-34: the metric function of a (case-insensitive) name (ValueError for an unknown one)."""
    name = metric_name.lower()
    if name not in DEFINED_METRICS:
        raise ValueError(f"Unknown metric: {metric_name}")
    return DEFINED_METRICS[name]


class EvalResult:
    """What ``ForecasterStep.evaluate`` returns (device tensors; B = batch, T = rollout, F = state variables, S = map steps):
    ``prediction`` (B, T, N, F), ``time_step_loss`` (T,), ``mean_loss`` (), ``entry_mse`` (B, T, F), and for phase "test"
    ``entry_mae`` (B, T, F), ``spatial_loss`` (B, S, N) at the 1-based ``map_steps`` (NaN off the interior) and, for a model
    that predicts its std, ``output_std`` (B, T, F); None where the phase does not produce it."""

    __slots__ = ("phase", "prediction", "time_step_loss", "mean_loss", "entry_mse", "entry_mae", "spatial_loss", "output_std",
                 "map_steps")

    def __init__(self, phase, prediction, time_step_loss, mean_loss, entry_mse, entry_mae=None, spatial_loss=None,
                 output_std=None, map_steps=()):
        self.phase, self.prediction, self.time_step_loss, self.mean_loss = phase, prediction, time_step_loss, mean_loss
        self.entry_mse, self.entry_mae, self.spatial_loss, self.output_std = entry_mse, entry_mae, spatial_loss, output_std
        self.map_steps = tuple(map_steps)

    @property
    def batch_size(self):
        return self.prediction.shape[0]


class ForecasterStep(nn.Module):
    """The training_step / loss lines of ``ForecasterModule`` (models/module.py)
    without Lightning: on-device standardisation (:326-367), rollout + masked
    loss per step (``wmse`` unless ``loss`` says otherwise), mean over batch then over steps (:463-510, :412)."""

    def __init__(self, forecaster: ARForecaster, datastore, standardize: bool = False, state_feature_weights=None,
                 loss: str = "wmse"):
        """``standardize=True`` makes ``forward`` start with ``on_after_batch_transfer`` (the batch arrives
        un-standardised, as ``WeatherDataset`` hands it over).  ``state_feature_weights``: per-variable loss weights
        (``get_state_feature_weighting``, module.py:162-176 / loss_weighting.py); default = uniform ``1 / n``.
        ``loss``: the reference's ``--loss`` (train_model.py:271-276, ``metrics.get_metric``, module.py:226), one of
        mse, mae, wmse, wmae, nll, crps_gauss (case-insensitive; ValueError otherwise).  The std of a loss is the model's
        predicted std (output_std) or the per-variable ``diff_std / sqrt(weight)``; mse and mae ignore it, and with it
        ``state_feature_weights``, because the reference replaces the std with ones."""
        super().__init__()
        from ._lib import LOSS_KINDS, LOSS_WMSE

        name = str(loss).lower()
        if name not in LOSS_KINDS:
            raise ValueError(f"unknown loss {loss!r}: expected one of {', '.join(LOSS_KINDS)}")
        self.loss_name, self.loss_kind = name, LOSS_KINDS[name]
        # wmse takes inv_var = 1 / std^2 where the kinds take the std: StepTailFunction with kind=None (the same kernels on another
        # loss term), and WmseLossFunction on the unfused route
        self.default_loss = self.loss_kind == LOSS_WMSE
        self.forecaster = forecaster
        self.standardize_inputs = bool(standardize)
        self.state_var_names = [str(n) for n in datastore.get_vars_names("state")]   # what EnsembleForecast(events=...) names
        bm = torch.tensor(datastore.boundary_mask.values, dtype=torch.float32)
        self.register_buffer("interior_mask_bool", (1.0 - bm).to(torch.bool), persistent=False)
        self.register_buffer("interior_index", torch.nonzero(1.0 - bm > 0.5).reshape(-1), persistent=False)
        interior = (1.0 - bm > 0.5).to(torch.float32)
        self.register_buffer("interior_weight", interior / interior.sum().clamp(min=1.0), persistent=False)
        st = datastore.get_standardization_dataarray("state")
        eps = torch.finfo(torch.float32).eps
        if not forecaster.predicts_std:
            n = len(datastore.get_vars_names("state"))
            if state_feature_weights is None:
                w = torch.tensor([1.0 / n] * n, dtype=torch.float32)  # loss_weighting.py:60-79 (uniform)
            else:   # ManualStateFeatureWeighting: one weight per state variable, in variable order
                w = torch.as_tensor(state_feature_weights, dtype=torch.float32).reshape(-1)
                if w.numel() != n or bool((w <= 0).any()):
                    raise ValueError(f"state_feature_weights needs {n} positive entries, got {tuple(w.shape)}")
            diff_std = torch.tensor(st.state_diff_std_standardized.values, dtype=torch.float32)
            self.register_buffer("per_var_std", diff_std / torch.sqrt(w), persistent=False)
            self.register_buffer("inv_var", 1.0 / (self.per_var_std * self.per_var_std), persistent=False)   # 1 / std^2 of wmse
        else:
            self.per_var_std = None
            self.inv_var = None
        self.register_buffer("state_mean", torch.tensor(st.state_mean.values, dtype=torch.float32), persistent=False)
        self.register_buffer(
            "state_std", torch.clamp(torch.tensor(st.state_std.values, dtype=torch.float32), min=eps), persistent=False
        )
        if datastore.get_num_data_vars("forcing") > 0:
            fs = datastore.get_standardization_dataarray("forcing")
            self.register_buffer("forcing_mean", torch.tensor(fs.forcing_mean.values, dtype=torch.float32), persistent=False)
            self.register_buffer(
                "forcing_std", torch.clamp(torch.tensor(fs.forcing_std.values, dtype=torch.float32), min=eps),
                persistent=False,
            )
        else:
            self.forcing_mean = self.forcing_std = None

    def standardization_stats(self):
        """The statistics ``on_after_batch_transfer`` uses (module.py:159-215; std clamped to eps, :306-324), in the form
        ``neural_lam_amd.data.DeviceWeatherDataset(standardization=...)`` takes to fold the hook into its batch launch."""
        d = {"state_mean": self.state_mean, "state_std": self.state_std}
        if self.forcing_mean is not None:
            d.update(forcing_mean=self.forcing_mean, forcing_std=self.forcing_std)
        return d

    def standardize(self, init_states, target_states, forcing, out=None):
        """module.py:326-367: one launch for the three tensors (``nlam_standardize``).  ``out``: three preallocated tensors
        (the trainer hands over the static inputs of its captured step: no separate staging copy of the batch)."""
        from .ops import standardize as std_launch

        items = [(init_states, self.state_mean, self.state_std, 1), (target_states, self.state_mean, self.state_std, 1)]
        has_forcing = forcing.shape[-1] > 0 and self.forcing_mean is not None
        if has_forcing:
            window = forcing.shape[-1] // self.forcing_mean.shape[-1]
            items.append((forcing, self.forcing_mean, self.forcing_std, window))
        outs = std_launch(items, None if out is None else list(out[: len(items)]))
        if not has_forcing and out is not None:
            out[2].copy_(forcing)
        return outs[0], outs[1], (outs[2] if has_forcing else (forcing if out is None else out[2]))

    def forward(self, init_states, target_states, forcing, standardize: bool | None = None):
        if standardize is None:
            standardize = self.standardize_inputs
        if standardize:
            init_states, target_states, forcing = self.standardize(init_states, target_states, forcing)
        if not self.default_loss or self._ext_tail(init_states, target_states):
            return self._forward_loss(init_states, target_states, forcing)
        if (self.inv_var is not None and init_states.is_cuda and FUSED_STATE_UPDATE and isinstance(self.forecaster, ARForecaster)):
            # rollout with every step's state update + boundary overwrite + loss term in one pass (one more in backward)
            B, T = target_states.shape[0], target_states.shape[1]
            prediction, pred_std, loss = self.forecaster(init_states, forcing, target_states,
                                                         loss_spec=(target_states, self.inv_var, self.interior_weight, 1.0 / (B * T)))
            if loss is not None:
                return prediction, loss
        else:
            prediction, pred_std = self.forecaster(init_states, forcing, target_states)
        if pred_std is None and prediction.is_cuda:
            # fixed per-variable std: wmse + interior mask + the grid / batch / step means in one HBM-bound kernel pair
            from .ops import WmseLossFunction

            return prediction, WmseLossFunction.apply(prediction, target_states, self.inv_var, self.interior_weight)
        if pred_std is None:
            pred_std = self.per_var_std
        time_step_loss = torch.mean(wmse(prediction, target_states, pred_std, mask=self.interior_index), dim=0)
        return prediction, torch.mean(time_step_loss)

    def _ext_tail(self, init_states, boundary_states) -> bool:
        """Whether the rollout of these inputs runs its tail on ops.StepTailExtFunction (ARForecaster.takes_ext_tail)."""
        return isinstance(self.forecaster, ARForecaster) and self.forecaster.takes_ext_tail(init_states, boundary_states)

    def _forward_loss(self, init_states, target_states, forcing):
        """Every ``loss`` but wmse: the fused step tail (ops.StepTailFunction with the kind) where the predictor can return its raw delta,
        ops.StepTailExtFunction for a clamped or predicted-std model (wmse included: the kind's entry on the per-variable or the
        predicted std), the one-pass ops.LossFunction on the rollout where neither applies (FUSED_CLAMPED_TAIL off)."""
        from ._lib import LOSS_MAE, LOSS_MSE
        from .ops import LossFunction

        fusable = self.per_var_std is not None or self._ext_tail(init_states, target_states)
        if fusable and init_states.is_cuda and FUSED_STATE_UPDATE and isinstance(self.forecaster, ARForecaster):
            B, T = target_states.shape[0], target_states.shape[1]
            prediction, pred_std, loss = self.forecaster(
                init_states, forcing, target_states,
                loss_spec=(target_states, self.per_var_std, self.interior_weight, 1.0 / (B * T), self.loss_kind))
            if loss is not None:
                return prediction, loss
        else:
            prediction, pred_std = self.forecaster(init_states, forcing, target_states)
        if self.loss_kind in (LOSS_MSE, LOSS_MAE):   # the reference's std of ones: neither std is read
            pred_std = None
        elif pred_std is not None:
            pred_std = pred_std.float()
        return prediction, LossFunction.apply(prediction.float(), target_states.float(), pred_std,
                                              self.per_var_std if pred_std is None else None, self.interior_weight, self.loss_kind)

    def evaluate(self, init_states, target_states, forcing, phase="val", steps_to_log=(1,), standardize=None):
        """``validation_step`` (phase "val", models/module.py:546-576) or ``test_step`` ("test", :607-681) without Lightning:
        the rollout under ``torch.no_grad()``, then every metric of the step in one ``nlam_eval_metrics`` pass (ops.eval_metrics)
        with this step's ``loss`` and its std.  ``steps_to_log``: the 1-based lead times of the test loss maps
        (``val_steps_to_log``); those beyond the rollout are skipped, as in the reference.  No host synchronisation and no
        data-dependent shape: the call can be captured (trainer.graphed_eval_step).  Returns an ``EvalResult``."""
        if phase not in ("val", "test"):
            raise ValueError(f"evaluate: phase must be 'val' or 'test', got {phase!r}")
        with torch.no_grad():
            if standardize is None:
                standardize = self.standardize_inputs
            if standardize:
                init_states, target_states, forcing = self.standardize(init_states, target_states, forcing)
            prediction, pred_std = self.forecaster(init_states, forcing, target_states)
            return EvalResult(*self._eval_fields(prediction, pred_std, target_states, phase, steps_to_log))

    def _eval_fields(self, prediction, pred_std, target_states, phase, steps_to_log):
        """The arguments of ``EvalResult`` for a finished rollout: every metric of the step in one ``nlam_eval_metrics`` pass."""
        from .ops import eval_metrics

        prediction = prediction.float().contiguous()
        if pred_std is not None:
            pred_std = pred_std.float().contiguous()
        T = prediction.shape[1]
        test = phase == "test"
        map_steps = tuple(int(k) for k in steps_to_log if int(k) <= T) if test else ()
        m = eval_metrics(prediction, target_states.float().contiguous(), pred_std, self.per_var_std, self.interior_weight,
                         self.loss_kind, [k - 1 for k in map_steps], want_mae=test, want_std=test and pred_std is not None)
        time_step_loss = torch.mean(m["step_loss"], dim=0)
        return (phase, prediction, time_step_loss, torch.mean(time_step_loss), m["sq"], m.get("ab"), m.get("maps"),
                m.get("std_mean"), map_steps)


class EFMForecaster(ARForecaster):
    """The rollout of the Graph-EFM training objective (Oskarsson et al. 2024, section 3) over a ``GraphEFM`` /
    ``GraphEFMMultiScale`` predictor.  Per AR step t:

        embed the grid and the static graph features (the static ones once per rollout, shared by prior, encoder and decoder)
        pp = predictor.prior_params(..)              pq = predictor.posterior_params(.., target_t, ..)
        z, kl_t = ops.LatentKLFunction(pq, pp, ..)   (z = mu_q + s_q eps; kl_t = kl_weight * sum_b KL(q || p))
        raw = decoder(z); new state, loss term = the step tail (rescale, clamps, predicted std, boundary overwrite)

    and the new state is the next step's ``prev_state``: the rollout follows posterior samples.  A subclass of ``ARForecaster``
    for what it shares (the masks, ``predicts_std``, being what ``forecast.EnsembleForecast`` accepts), a ``forward`` of its own:
    ``ARForecaster.forward`` keeps Graph-EFM off the fused tails and is untouched.

    The static embeddings are not registered for the rollout-shared gradient hand-over (``ops.rollout_shared_reset``): that
    hand-over serves one fused edge launch per AR step, here a step has up to three consumers of an embedding (prior, encoder,
    decoder), one of which a constant prior drops, so autograd adds their gradients as it does for ``ForecasterStep`` over a
    Graph-EFM.  ``forward`` clears whatever another model registered."""

    def forward(self, init_states, forcing_features, boundary_states, loss_spec=None, kl_words=None, latent_noise=None):
        """``loss_spec = (target_states, var_std (F,) | None, row_weight (N,), scale, kind)`` as ``ARForecaster.forward`` takes
        it; ``kl_words = (kl_weight, seed, draw)``, the device words of ``EFMForecasterStep``; ``latent_noise`` (B, T, R, D):
        standard-normal noise in place of the generator's.  Returns (prediction (B, T, N, F), pred_std | None, likelihood,
        kl): the two terms of the loss, weights included; ``self.last_kl`` keeps the unweighted (T, B) KL per item.  Without
        ``kl_words`` this is ``ARForecaster.forward`` (a rollout on samples of the prior; what ``ForecasterStep`` calls)."""
        from .ops import LatentKLFunction, LossFunction, StepTailExtFunction, StepTailFunction, rollout_shared_reset

        if kl_words is None:   # not the objective: ARForecaster's rollout on samples of the prior, as for any step predictor
            return super().forward(init_states, forcing_features, boundary_states, loss_spec)
        if loss_spec is None or len(loss_spec) != 5:
            raise ValueError("EFMForecaster: the objective (kl_words given) needs the five-entry loss_spec of EFMForecasterStep")
        pred = self.predictor
        target, consts, row_weight, scale, kind = loss_spec
        kl_weight, seed, draw = kl_words
        prev_prev_state, prev_state = init_states[:, 0], init_states[:, 1]
        no_clamp = pred.clamp_tables() is None
        raw = (FUSED_STATE_UPDATE and init_states.is_cuda and init_states.dtype == torch.float32
               and boundary_states.dtype == torch.float32 and pred.can_return_raw_delta())
        plain = raw and no_clamp and not pred.output_std
        bmask = self.boundary_mask.reshape(-1)
        preds, stds, losses, kls, kl_items = [], [], [], [], []
        rollout_shared_reset(())
        with pred.static_cache():
            for i in range(forcing_features.shape[1]):
                forcing = forcing_features[:, i]
                grid_prev_emb, graph_emb = pred.embedd_grid_and_graph(prev_state, prev_prev_state, forcing)
                pp = pred.prior_params(grid_prev_emb, graph_emb)
                pq = pred.posterior_params(prev_state, prev_prev_state, forcing, target[:, i], graph_emb)
                z, kl_t, kl_b = LatentKLFunction.apply(pq.float(), pp.float(), kl_weight, seed, draw, i,
                                                       None if latent_noise is None else latent_noise[:, i])
                kls.append(kl_t)
                kl_items.append(kl_b)
                if raw:
                    delta, _ = pred.decode(grid_prev_emb, graph_emb, z, prev_state, raw_delta=True)
                    if plain:
                        new_state, loss_t = StepTailFunction.apply(delta.float(), prev_state, boundary_states[:, i], target[:, i],
                                                                   pred.diff_std, pred.diff_mean, bmask, consts, row_weight, scale, kind)
                        pred_std = None
                    else:
                        new_state, pred_std, loss_t = StepTailExtFunction.apply(
                            delta.float(), prev_state, boundary_states[:, i], target[:, i], pred.diff_std, pred.diff_mean, bmask,
                            consts, row_weight, scale, kind, pred.clamp_tables())
                    losses.append(loss_t)
                else:
                    pred_state, pred_std = pred.decode(grid_prev_emb, graph_emb, z, prev_state)
                    new_state = self.boundary_mask * boundary_states[:, i] + self.interior_mask * pred_state
                preds.append(new_state)
                if pred_std is not None:
                    stds.append(pred_std)
                prev_prev_state, prev_state = prev_state, new_state

        def _stack(xs):
            return xs[0].unsqueeze(1) if len(xs) == 1 else torch.stack(xs, dim=1)

        prediction, pred_std = _stack(preds), (_stack(stds) if stds else None)
        if losses:
            lik = losses[0] if len(losses) == 1 else torch.stack(losses).sum()
        else:   # the unfused tail: one loss pass over the rollout (its scale is the same 1 / (B T))
            from ._lib import LOSS_MAE, LOSS_MSE

            std = None if kind in (LOSS_MSE, LOSS_MAE) or pred_std is None else pred_std.float()
            lik = LossFunction.apply(prediction.float(), target.float(), std, consts if std is None else None, row_weight, kind)
        kl = kls[0] if len(kls) == 1 else torch.stack(kls).sum()
        self.last_kl = torch.stack(kl_items).detach()
        return prediction, pred_std, lik, kl

    last_kl = None

    def member_crps(self, init_states, forcing_features, boundary_states, target_states, members, crps_spec, seed, draw,
                    member_noise=None):
        """The ensemble CRPS term of the fine-tuning stage: a rollout of ``B * members`` items on samples of the PRIOR -- item
        ``b * members + m`` is member m of batch item b, started from that item's ``init_states`` under its forcing and boundary,
        each member fed its own new state -- and, per AR step, the unbiased ensemble CRPS of the members' new states against the
        target.  ``crps_spec = (var_weight (F,) | None, row_weight (N,), weight)``, ``weight`` the device float ``crps_weight / (B
        T)``; ``seed`` / ``draw``: the device words of the member draws; ``member_noise`` (B * members, T, R, D) replaces the
        generator.  The step tails run without a loss term (``target=None`` of ops.StepTailExtFunction); a predicted std of the
        members is not used.  Returns (term, crps_per_item (T, B) unweighted)."""
        from .ops import CrpsEnsFunction, LatentDrawFunction, StepTailExtFunction, crps_ens_torch

        pred = self.predictor
        M = int(members)
        var_weight, row_weight, weight = crps_spec
        rep = lambda x: x.repeat_interleave(M, dim=0)   # noqa: E731  member-minor: b * M + m
        init, forcing_m, boundary_m = rep(init_states), rep(forcing_features), rep(boundary_states)
        prev_prev_state, prev_state = init[:, 0], init[:, 1]
        raw = (FUSED_STATE_UPDATE and init.is_cuda and init.dtype == torch.float32 and boundary_m.dtype == torch.float32
               and pred.can_return_raw_delta())
        bmask = self.boundary_mask.reshape(-1)
        D = int(pred.latent_dim)
        terms, items = [], []
        with pred.static_cache():
            for i in range(forcing_m.shape[1]):
                forcing = forcing_m[:, i]
                grid_prev_emb, graph_emb = pred.embedd_grid_and_graph(prev_state, prev_prev_state, forcing)
                pp = pred.prior_params(grid_prev_emb, graph_emb)
                z = LatentDrawFunction.apply(pp.float(), D, seed, draw, i, None if member_noise is None else member_noise[:, i])
                if raw:
                    delta, _ = pred.decode(grid_prev_emb, graph_emb, z, prev_state, raw_delta=True)
                    new_state, _, _ = StepTailExtFunction.apply(delta.float(), prev_state, boundary_m[:, i], None, pred.diff_std,
                                                                pred.diff_mean, bmask, None, None, 1.0, None, pred.clamp_tables())
                else:
                    pred_state, _ = pred.decode(grid_prev_emb, graph_emb, z, prev_state)
                    new_state = self.boundary_mask * boundary_m[:, i] + self.interior_mask * pred_state
                if FUSED_CRPS:
                    term, per_item = CrpsEnsFunction.apply(new_state.float(), target_states[:, i].float(), row_weight, var_weight, weight, M)
                else:
                    term, per_item = crps_ens_torch(new_state.float(), target_states[:, i].float(), row_weight, var_weight, weight, M)
                terms.append(term)
                items.append(per_item)
                prev_prev_state, prev_state = prev_state, new_state
        crps = terms[0] if len(terms) == 1 else torch.stack(terms).sum()
        return crps, torch.stack(items).detach()


class EFMEvalResult(EvalResult):
    """What ``EFMForecasterStep.evaluate`` returns: the ``EvalResult`` of the rollout on posterior samples (``prediction``,
    ``time_step_loss`` .. as ``ForecasterStep.evaluate`` gives them, so ``evaluation.MetricAggregator`` and
    ``trainer.graphed_eval_step`` take it), and the validation ELBO ``loss`` = ``likelihood`` + ``kl`` (both weighted as in
    training), ``kl_per_item`` (T, B) unweighted, ``pred_std`` (B, T, N, F) or None.  A step with ``crps_members > 0`` adds its
    weighted ensemble CRPS term ``crps`` (from a member rollout on prior samples) to ``loss``; otherwise ``crps`` is None."""

    __slots__ = ("pred_std", "loss", "likelihood", "kl", "kl_per_item", "crps")

    def __init__(self, fields, pred_std, loss, likelihood, kl, kl_per_item, crps=None):
        super().__init__(*fields)
        self.pred_std, self.loss, self.likelihood, self.kl, self.kl_per_item = pred_std, loss, likelihood, kl, kl_per_item
        self.crps = crps


class EFMForecasterStep(ForecasterStep):
    """The training step of Graph-EFM: ``forward(init, target, forcing) -> (prediction, loss)`` with

        loss = 1 / (B T) sum_{b,t} [ lik_{b,t} + kl_beta / N_interior * KL_{b,t} ]

    ``lik`` the step tail's loss term of kind ``loss`` (``nll`` by default) under the conventions of ``ForecasterStep`` (interior
    mask, grid mean, sum over variables; the predicted std or the per-variable ``diff_std / sqrt(weight)``), ``KL`` the divergence
    of the encoder's posterior from the prior, summed over the latent.  This is the paper's negative ELBO (``-log p + beta KL``,
    summed over the grid) divided by the constant ``N_interior``: the same minimiser, the magnitude of ``--loss nll``, and the
    step tails run unchanged with their ``scale``.  Standardisation, the per-variable std and the loss names are
    ``ForecasterStep``'s (this is a subclass), so ``Trainer(step)`` takes it as it is.

    Noise.  The step owns three kinds of device words: ``seed`` (the 64-bit Philox key -- the C-ABI's uint64, kept in an int64
    buffer that carries the same 64 bits), ``draw`` (int64) and ``kl_weight`` (float, ``kl_beta / (N_interior B T)``: one word
    per batch shape, ``kl_weight_word(B, T)``, so that an eager step or an ``evaluate`` at another shape never changes what a
    recorded step reads).  Every ``forward`` advances ``draw`` by one on the device before its first draw, and the
    draw of AR step t, item b is keyed by (seed; quad, t, b, draw): a replay of the captured step draws new noise and records
    nothing again; so does every micro-batch of an accumulation window.  ``set_kl_beta`` (annealing) and ``reseed`` write the
    words in place.  Ranks must not share noise: the key is ``noise_key(seed, rank) = (seed + rank * 0x9E3779B97F4A7C15) mod 2^64``
    (an odd multiplier: distinct ranks give distinct keys), ``rank`` from ``torch.distributed`` unless given.
    ``draw_state()`` / ``load_draw_state()`` carry ``{seed, draw, kl_beta}`` through ``save_checkpoint(..., extra=...)``.
    ``last_terms``: the device scalars (likelihood, kl) of the last forward that ran, eager or replayed.

    The fine-tuning stage (the paper's ``L_Var + lambda_CRPS L_CRPS``).  ``crps_members = M`` (2 .. 16; 0, the default, leaves the
    step as described above, launch for launch) makes every ``forward`` run, behind the ELBO rollout, ``EFMForecaster.member_crps``:
    M members per batch item rolled out on samples of the prior, and

        loss = lik + kl + crps_weight / (B T) sum_{b,t} sum_n w_n sum_f c_f [ 1/M sum_m |x_m - y| - 1/(M (M-1)) sum_{i<j} |x_i - x_j| ]

    ``w_n`` the interior weight, ``c_f = 1 / per_var_std[f]`` as ``wmae`` weights (ones with a predicted std), x_m member m's new
    state, y the target.  ``crps_weight / (B T)`` is a device float per batch shape like ``kl_weight`` (``crps_weight_word``,
    ``set_crps_weight``: in place, nothing recorded again; a weight of 0 still runs the members).  The members draw on the same
    ``draw`` word under a key of their own, ``member_key(seed, rank) = (noise_key + 0xD1B54A32D192ED03) mod 2^64``, with counter
    (quad, t, b M + m, low word of draw): posterior and member draws never share a (key, counter) pair.  ``last_crps``: the
    weighted term of the last forward.  ``draw_state()`` then carries ``crps_weight`` too.  The member rollout keeps M times the
    activations of the ELBO rollout alive for the backward."""

    MEMBER_KEY_OFFSET = 0xD1B54A32D192ED03

    def __init__(self, forecaster, datastore, standardize: bool = False, state_feature_weights=None, loss: str = "nll",
                 kl_beta: float = 1.0, seed: int = 0, rank: int | None = None, crps_members: int = 0, crps_weight: float = 0.0):
        if not getattr(getattr(forecaster, "predictor", None), "draws_latent", False):
            raise ValueError(f"EFMForecasterStep trains a predictor that draws a latent variable (GraphEFM, GraphEFMMultiScale), not "
                             f"{type(getattr(forecaster, 'predictor', forecaster)).__name__}: use ForecasterStep")
        if not isinstance(forecaster, EFMForecaster):
            raise ValueError("EFMForecasterStep needs an EFMForecaster over the predictor")
        from ._lib import CRPS_MAX_MEMBERS

        crps_members = int(crps_members)
        if crps_members != 0 and not 2 <= crps_members <= CRPS_MAX_MEMBERS:
            raise ValueError(f"EFMForecasterStep: crps_members must be 0 (no CRPS term) or 2 .. {CRPS_MAX_MEMBERS}, got {crps_members}")
        if crps_members == 0 and float(crps_weight) != 0.0:
            raise ValueError("EFMForecasterStep: crps_weight without crps_members: the CRPS term needs at least 2 members")
        super().__init__(forecaster, datastore, standardize=standardize, state_feature_weights=state_feature_weights, loss=loss)
        if rank is None:
            import torch.distributed as dist

            rank = dist.get_rank() if dist.is_available() and dist.is_initialized() else 0
        self.rank = int(rank)
        self.n_interior = int(self.interior_index.numel())
        self.kl_beta, self.seed_value = float(kl_beta), int(seed) & 0xFFFFFFFFFFFFFFFF
        self.register_buffer("seed", torch.zeros((1,), dtype=torch.int64), persistent=False)      # the 64 bits of the key
        self.register_buffer("draw", torch.zeros((1,), dtype=torch.int64), persistent=False)
        self.register_buffer("eval_draw", torch.full((1,), 1 << 31, dtype=torch.int64), persistent=False)
        self.register_buffer("_terms", torch.zeros((2,), dtype=torch.float32), persistent=False)   # (likelihood, kl) of the last forward
        self._kl_words = {}   # (B, T) -> the device float kl_beta / (N_interior B T) of the steps recorded or run at that shape
        self._seed_device = None
        self.crps_members, self.crps_weight = crps_members, float(crps_weight)
        self._crps_words = {}   # (B, T) -> the device float crps_weight / (B T), kept as _kl_words is
        if crps_members:
            self.register_buffer("member_seed", torch.zeros((1,), dtype=torch.int64), persistent=False)   # the members' key
            self.register_buffer("_crps_term", torch.zeros((), dtype=torch.float32), persistent=False)
            self.register_buffer("crps_var_weight", None if self.per_var_std is None else 1.0 / self.per_var_std, persistent=False)

    @property
    def last_crps(self):
        """The weighted CRPS term of the last ``forward`` that ran, eager or replayed: a device scalar of its own (None without
        members)."""
        return self._crps_term if self.crps_members else None

    @classmethod
    def member_key(cls, seed: int, rank: int) -> int:
        """The Philox key of the member draws of ``rank`` under ``seed``: the posterior's key plus an odd constant."""
        return (cls.noise_key(seed, rank) + cls.MEMBER_KEY_OFFSET) & 0xFFFFFFFFFFFFFFFF

    def crps_weight_value(self, B: int, T: int) -> float:
        """``crps_weight / (B T)``: what the host writes into the device word of that batch shape."""
        return self.crps_weight / (B * T)

    def crps_weight_word(self, B: int, T: int):
        """The device float ``crps_weight / (B T)`` of batch shape (B, T): ``kl_weight_word``'s rules -- one word per shape, made
        on first use outside a capture, then only written in place (``set_crps_weight``)."""
        self.kl_weight_word(B, T)   # the device check (drops the words of another device, writes the keys), and the same error
        word = self._crps_words.get((B, T))
        if word is None:
            dev = self.draw.device
            if dev.type == "cuda" and torch.cuda.is_current_stream_capturing():
                raise RuntimeError("EFMForecasterStep: the first call for a batch shape must run outside a stream capture (Trainer's "
                                   "warm-up does): it writes that shape's crps_weight")
            word = self._crps_words[(B, T)] = torch.full((1,), self.crps_weight_value(B, T), dtype=torch.float32, device=dev)
        return word

    def set_crps_weight(self, crps_weight: float):
        """A new ``crps_weight``, written in place into the device word of every batch shape seen so far: no captured step is
        recorded again.  Not between a ``forward`` and its ``backward`` (as ``set_kl_beta``)."""
        if not self.crps_members:
            raise ValueError("EFMForecasterStep.set_crps_weight: the step was built without crps_members")
        self.crps_weight = float(crps_weight)
        for (B, T), word in self._crps_words.items():
            word.fill_(self.crps_weight_value(B, T))

    @property
    def last_terms(self):
        """(likelihood, kl) of the last ``forward`` that ran -- eager or a replay of a recorded one: views of a device buffer the
        forward writes, weights included, no gradient."""
        return self._terms[0], self._terms[1]

    @staticmethod
    def noise_key(seed: int, rank: int) -> int:
        """The Philox key of ``rank`` under ``seed``: 64 bits, distinct for distinct ranks."""
        return (int(seed) + int(rank) * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF

    def kl_weight_value(self, B: int, T: int) -> float:
        """``kl_beta / (N_interior B T)``: what the host writes into the device word of that batch shape."""
        return self.kl_beta / (self.n_interior * B * T)

    def kl_weight_word(self, B: int, T: int):
        """The device float ``kl_beta / (N_interior B T)`` of batch shape (B, T): one word per shape, because a recorded step keeps
        reading the word it was recorded with (its ``1 / (B T)`` is baked into the tails' ``scale`` in the same way) while an
        eager call or ``evaluate`` at another shape runs in between.  Made on first use and then only written in place
        (``set_kl_beta``); never made inside a capture: the recorded fill would undo ``set_kl_beta`` at every replay."""
        dev = self.draw.device
        if self._seed_device != dev:   # after construction / ``.to()``: the words of another device are dropped, the key is written
            self._kl_words, self._crps_words = {}, {}
            self._write_seed()
        word = self._kl_words.get((B, T))
        if word is None:
            if dev.type == "cuda" and torch.cuda.is_current_stream_capturing():
                raise RuntimeError("EFMForecasterStep: the first call for a batch shape must run outside a stream capture (Trainer's "
                                   "warm-up does): it writes that shape's kl_weight")
            word = self._kl_words[(B, T)] = torch.full((1,), self.kl_weight_value(B, T), dtype=torch.float32, device=dev)
        return word

    def _write_seed(self):
        key = self.noise_key(self.seed_value, self.rank)
        self.seed.fill_(key - (1 << 64) if key >= (1 << 63) else key)   # the 64 bits, in the int64 the device word is kept as
        if self.crps_members:
            key = self.member_key(self.seed_value, self.rank)
            self.member_seed.fill_(key - (1 << 64) if key >= (1 << 63) else key)
        self._seed_device = self.seed.device

    def set_kl_beta(self, kl_beta: float):
        """A new ``kl_beta`` (annealing), written in place into the device word of every batch shape seen so far: no captured step
        is recorded again.  Not between a ``forward`` and its ``backward``: the operator saved the word (autograd then refuses)."""
        self.kl_beta = float(kl_beta)
        for (B, T), word in self._kl_words.items():
            word.fill_(self.kl_weight_value(B, T))

    def reseed(self, seed: int, draw: int = 0):
        """A new seed and draw count, written in place (no new recording): the next call draws (seed, draw + 1)."""
        self.seed_value = int(seed) & 0xFFFFFFFFFFFFFFFF
        if self._seed_device != self.draw.device:
            self._kl_words, self._crps_words = {}, {}
        self._write_seed()
        self.draw.fill_(int(draw))

    def draw_state(self) -> dict:
        """``{seed, draw, kl_beta}`` for ``save_checkpoint(..., extra=step.draw_state())`` (reads ``draw`` back: synchronises)."""
        state = {"seed": self.seed_value, "draw": int(self.draw.item()), "kl_beta": self.kl_beta}
        if self.crps_members:
            state["crps_weight"] = self.crps_weight
        return state

    def load_draw_state(self, state: dict):
        """Continue the noise sequence of a saved run (the rank's key is folded in again here)."""
        self.reseed(int(state["seed"]), int(state["draw"]))
        self.set_kl_beta(float(state["kl_beta"]))
        if self.crps_members and "crps_weight" in state:
            self.set_crps_weight(float(state["crps_weight"]))

    def replay_state(self):
        """The device counters ``forward`` advances: ``Trainer`` puts them back behind the warm-up passes of a recording."""
        return [self.draw]

    def _elbo(self, init_states, target_states, forcing, draw, latent_noise):
        B, T = target_states.shape[0], target_states.shape[1]
        kl_weight = self.kl_weight_word(B, T)
        if latent_noise is None:
            draw.add_(1)
        spec = (target_states, self.per_var_std, self.interior_weight, 1.0 / (B * T), self.loss_kind)
        return self.forecaster(init_states, forcing, target_states, loss_spec=spec, kl_words=(kl_weight, self.seed, draw),
                               latent_noise=latent_noise)

    def _crps(self, init_states, target_states, forcing, draw, member_noise):
        """The weighted CRPS term of a member rollout on prior samples under ``draw`` as ``_elbo`` left it (the members share the
        posterior's draw count and differ in the key)."""
        B, T = target_states.shape[0], target_states.shape[1]
        spec = (self.crps_var_weight, self.interior_weight, self.crps_weight_word(B, T))
        crps, _ = self.forecaster.member_crps(init_states, forcing, target_states, target_states, self.crps_members, spec,
                                              self.member_seed, draw, member_noise)
        return crps

    def forward(self, init_states, target_states, forcing, standardize: bool | None = None, latent_noise=None, member_noise=None):
        """``member_noise`` (B * crps_members, T, R, D): standard-normal noise of the member rollout in place of the generator's.
        Without it the members draw under ``draw`` as it stands, which only a call without ``latent_noise`` advances."""
        if standardize is None:
            standardize = self.standardize_inputs
        if standardize:
            init_states, target_states, forcing = self.standardize(init_states, target_states, forcing)
        prediction, _, lik, kl = self._elbo(init_states, target_states, forcing, self.draw, latent_noise)
        torch.stack((lik.detach().reshape(()), kl.detach().reshape(())), out=self._terms)   # one launch, recorded with the step
        if not self.crps_members:
            return prediction, lik + kl
        crps = self._crps(init_states, target_states, forcing, self.draw, member_noise)
        self._crps_term.copy_(crps.detach().reshape(()))
        return prediction, lik + kl + crps

    def evaluate(self, init_states, target_states, forcing, phase="val", steps_to_log=(1,), standardize=None, latent_noise=None,
                 member_noise=None):
        """``ForecasterStep.evaluate`` for this objective: the launches of ``forward`` under ``torch.no_grad()`` -- the rollout on
        posterior samples -- then the metric pass of ``validation_step`` / ``test_step`` on its predictions.  Returns an
        ``EFMEvalResult``: the ``EvalResult`` fields plus the validation ELBO and its two terms.  It draws on a counter of its own
        (``eval_draw``, started at 2^31), so validating does not move the training run's noise sequence, and reads the
        ``kl_weight`` word of its own batch shape.  Capturable after one eager call at that shape (trainer.graphed_eval_step).
        With ``crps_members > 0`` the member rollout runs too, on ``eval_draw`` under the members' key: ``crps`` is its weighted term
        and ``loss`` includes it (``member_noise`` as in ``forward``)."""
        if phase not in ("val", "test"):
            raise ValueError(f"evaluate: phase must be 'val' or 'test', got {phase!r}")
        with torch.no_grad():
            if standardize is None:
                standardize = self.standardize_inputs
            if standardize:
                init_states, target_states, forcing = self.standardize(init_states, target_states, forcing)
            prediction, pred_std, lik, kl = self._elbo(init_states, target_states, forcing, self.eval_draw, latent_noise)
            fields = self._eval_fields(prediction, pred_std, target_states, phase, steps_to_log)
            if not self.crps_members:
                return EFMEvalResult(fields, pred_std, lik + kl, lik, kl, self.forecaster.last_kl)
            crps = self._crps(init_states, target_states, forcing, self.eval_draw, member_noise)   # the members on eval_draw too
            return EFMEvalResult(fields, pred_std, lik + kl + crps, lik, kl, self.forecaster.last_kl, crps)
