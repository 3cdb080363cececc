"""Autoregressive validation rollout on the libmgn inference kernels.

Semantics = the reference's LightningModule validation path:
  build_mask            lightning_module.py:17-25  (nodes that are neither NORMAL nor OUTFLOW keep
                                                    their ground truth)
  _make_prediction      lightning_module.py:168-202 (feed the previous prediction back into
                                                    x[:, output_index_start:end]; optional
                                                    previous-data channel; no_grad forward;
                                                    predicted[mask] = target[mask])
  validation_step loss  lightning_module.py:204-232 (masked L2 over NORMAL ∪ OUTFLOW)
  all-rollout RMSE      lightning_module.py:236-249 (sqrt(mean((pred − target)²)) over every step)
  trajectory reset      lightning_module.py:163-166

The forward runs in no-grad mode, so GraphNetBlocks use mgn_block_forward's inference kernels (no
backward saves). With graph=True the per-step work after the first step of a trajectory — write
the previous prediction into the static input, Simulator eval forward, mask, keep the prediction —
is one hipGraph replay; the host only copies the next frame's x and y into the static buffers.
Masking uses torch.where (the reference's boolean index_put would synchronise with the host). The
graph is re-recorded when the mesh (edge_index) changes.

With feed=ResidentTrajectories (dataset/resident.py), rollout_resident runs a whole trajectory from frames kept
on the device as one replay per step of a single captured graph: libmgn's mgn_rollout_begin (frame start + s,
the previous prediction fed back when s > 0), the same Simulator eval forward, mgn_rollout_end (mask, feedback
state, the kept prediction, the step's loss and squared error, s += 1). The step counter s lives on the device;
the host neither builds per-frame batches nor keeps lists of predictions, and never synchronises.

Lagrangian data (a feed built with world_pos=, e.g. DeformingPlate): Rollout(..., world_edges=MODE) runs the same
three stages with mgn_rollout_begin_world in front — the batch row [world(3), obstacle displacement(3), the other
columns] of frame start + s built from clean values, then the feedback in batch-layout columns, as the
reference's validation does (its dataset item is built first, _make_prediction writes the prediction back after
it: the displacement is never recomputed) — plus one mgn_feed_world_edge_features launch for the four world
columns of edge_attr. MODE says which positions those follow, and the caller must choose: "frame", the clean
world positions of frame start + s (the reference's validation: its edge features are part of the dataset item);
"prediction", the x the model is about to see, so from step 1 on the fed-back positions; "off", x only (models
without edge_attr, feeds without an edge side). The default None refuses such a feed.

World edges that change from frame to frame (a feed built with dynamic_edges=, the transformer configs such as
plate.json): the same modes say which positions the reference's add_world_edges reads — "frame", the clean world
positions of frame start + s (the reference's validation: its edge_index is part of the dataset item), "prediction",
the x the model is about to see — and one mgn_world_topology_build between the begin stage and the forward rebuilds
the feed's bound topology in place, inside the recorded step. "off" is refused: there is no static adjacency to
fall back to. batch.edge_index must be feed.edge_index; the steps' edge counts are kept in resident_num_edges. On a
feed that has random_edges= as well, the same build_edges is mgn_world_random_topology_build with the feed's current
pairs and random_enabled word: the rollout draws nothing, and after feed.set_random_edges(False) — what the reference's
validation, which adds no random edges, amounts to — it equals the rollout of a dynamic_edges=-only feed.

Aneurysm data (a feed built with aneurysm=): Rollout(..., acceleration=MODE) runs the same three stages with
mgn_rollout_begin_aneurysm in front — the row [frame row (F) ‖ a − p ‖ pos ‖ mean, min, max ‖ node type] of the
reference's external/aneurysm.py build_features at frame start + s, from clean values, then the feedback, as the
reference's validation does (the dataset item is built first, _make_prediction writes into it afterwards). MODE says
what the acceleration columns [F, F + 3) hold from step 1 on, and the caller must choose, because the reference's
own default (use_previous_data=False) would feed ground-truth accelerations to a model that predicts velocities:
"frame", the clean a − p of every step (the reference with use_previous_data=False); "prediction", the previous
step's predicted − current, i.e. the acceleration columns are the previous-data columns (the reference's train.py
default, use_previous_data=True with columns 4, 7 on F = 4). The inflow statistics are those of the clean frames in
both modes: INFLOW rows are masked back to the target on every step, so the prediction would give the same values.
Start frames lie in [1, T − 2] (frame start − 1 is read). The default None refuses such a feed.
"""
import math
import weakref

import torch

from graphphysics.utils.loss import masked_mse
from graphphysics.utils.nodetype import NodeType


def build_mask(param, graph):
    """True on nodes whose prediction is replaced by the target (reference lightning_module.py:17-25).
    param: the reference's parameter dict ({"index": {"node_type_index": k}}) or the index itself."""
    k = param["index"]["node_type_index"] if isinstance(param, dict) else int(param)
    node_type = graph.x[:, 0, k] if graph.x.dim() > 2 else graph.x[:, k]
    return torch.logical_not(torch.logical_or(node_type == NodeType.NORMAL, node_type == NodeType.OUTFLOW))


class _Frame:
    """Attribute bag standing in for the cloned PyG batch (x, y, edge_index, edge_attr, pos)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


class _Resident:
    """The device state of rollout_resident for one mesh and shape: the static batch the graph reads, the
    feedback state, the result buffers and the step counter."""


class Rollout:
    def __init__(self, sim, node_type_index, masks=(NodeType.NORMAL, NodeType.OUTFLOW), use_previous_data=False,
                 previous_data_start=None, previous_data_end=None, graph=True, feed=None, world_edges=None,
                 acceleration=None):
        self.sim = sim
        self.k = int(node_type_index)
        self.masks = list(masks)
        self.use_prev = use_previous_data
        self.ps, self.pe = previous_data_start, previous_data_end
        self.use_graph = graph
        self.os, self.oe = sim.output_index_start, sim.output_index_end
        self._graph = None
        self._key = None
        self.outputs, self.targets, self.losses = [], [], []
        # feed (dataset.resident.ResidentTrajectories): the trajectories rollout_resident reads. A validation
        # feed of its own: set_frames puts it into explicit mode, a TrainStep sharing it would re-record.
        self.feed = feed
        # world_edges: None, or for a feed built with world_pos= where the world columns of edge_attr come from:
        # "frame" (the clean frame), "prediction" (the x the model sees) or "off" (module docstring)
        self.world_edges = world_edges
        # acceleration: None, or for a feed built with aneurysm= what the acceleration columns hold from step 1 on:
        # "frame" (the clean frames) or "prediction" (the previous-data channel) (module docstring)
        self.acceleration = acceleration
        self._given_prev = (use_previous_data, previous_data_start, previous_data_end)  # as the caller wrote them
        self._res = None  # rollout_resident's state (_Resident)
        self.resident_records = 0  # how many times rollout_resident recorded its graph
        self._res_sq, self._res_count = [], 0  # Σ (pred − target)² per resident run (device), and their elements
        self.resident_num_edges = None  # rollout_resident on a dynamic_edges= feed: the steps' edge counts
        if feed is not None:
            from graphphysics.dataset.resident import check_rollout_columns

            self._refuse_aneurysm_without_mode(feed)
            world = self._check_world(feed)
            if torch.device(sim.device).type != feed.traj.device.type:
                raise ValueError(f"feed lives on {feed.traj.device}, the simulator on {sim.device}")
            # an aneurysm= feed: _check_acceleration sets use_prev and the columns and checks them against F + 10
            if not self._check_acceleration(feed):
                self._prev_cols = (int(self.ps), int(self.pe)) if self.use_prev else None
                # a world feed: the batch row is 3 wider than the frame's, every index here is in batch layout
                check_rollout_columns(feed.F + 3 if world else feed.F, feed.y_columns, (self.os, self.oe),
                                      self._prev_cols, self.k)
        elif acceleration is not None:
            raise ValueError(f"acceleration={acceleration!r} needs feed=, a ResidentTrajectories built with aneurysm=")
        self.reset()

    ACCELERATION = ("frame", "prediction")

    def _refuse_aneurysm_without_mode(self, feed):
        if getattr(feed, "aneurysm", False) and self.acceleration is None:
            raise ValueError("the resident rollout of a feed built with aneurysm= is not supported yet without "
                             'Rollout(..., acceleration="frame" | "prediction"), which says whether the acceleration '
                             "columns follow the clean frames or the previous prediction; a default is left to a "
                             "later pull request")

    def _check_acceleration(self, feed):
        """ValueError unless acceleration= fits the feed and the columns; returns whether the feed was built with
        aneurysm=. For such a feed this (re)derives use_prev, the previous-data columns and _prev_cols from what
        the caller gave and the mode, so a mode changed after construction is applied by the next run."""
        aneurysm, mode = bool(getattr(feed, "aneurysm", False)), self.acceleration
        if mode is not None and mode not in self.ACCELERATION:
            raise ValueError(f"acceleration must be None or one of {self.ACCELERATION}, got {mode!r}")
        if mode is not None and self.world_edges is not None:
            raise ValueError("acceleration= and world_edges= do not go together: a feed is built with aneurysm= or "
                             "with world_pos=, never both")
        if not aneurysm:
            if mode is not None:
                raise ValueError(f"acceleration={mode!r} needs a feed built with aneurysm=")
            return False
        self._refuse_aneurysm_without_mode(feed)
        from graphphysics.dataset.resident import check_rollout_columns

        F = feed.F
        if self.k != F + 9:
            raise ValueError(f"node_type_index {self.k} differs from F + 9 = {F + 9}, the node-type column of the "
                             "row an aneurysm= feed writes")
        use, ps, pe = self._given_prev
        acc = (F, F + 3)
        if mode == "prediction":
            if (self.os, self.oe) != (0, 3):
                raise ValueError(f'acceleration="prediction" needs the output columns (0, 3), the velocity whose '
                                 f"step-to-step difference the acceleration columns hold; got ({self.os}, {self.oe})")
            if not use:
                use, ps, pe = True, acc[0], acc[1]
            elif (int(ps), int(pe)) != acc:
                raise ValueError(f'acceleration="prediction" makes the acceleration columns {acc} the previous-data '
                                 f"columns; got previous-data columns ({ps}, {pe})")
        elif use and int(ps) < acc[1] and acc[0] < int(pe):
            raise ValueError(f'acceleration="frame" keeps the acceleration columns {acc} on the clean frames, but the '
                             f'previous-data columns ({ps}, {pe}) intersect them; use acceleration="prediction"')
        self.use_prev, self.ps, self.pe = use, ps, pe
        self._prev_cols = (int(ps), int(pe)) if use else None
        check_rollout_columns(F + 10, feed.y_columns, (self.os, self.oe), self._prev_cols, self.k)
        return True

    WORLD_EDGES = ("frame", "prediction", "off")

    def _check_world(self, feed):
        """ValueError unless world_edges fits the feed; returns whether the feed was built with world_pos=. The
        resident rollout of a plain feed reads the frames in frame layout; a world_pos= feed trains on rows that
        are 3 columns wider (the obstacle displacement), and its rollout has to be told where the world columns
        of edge_attr come from."""
        world, mode = bool(getattr(feed, "world", False)), self.world_edges
        if mode is not None and mode not in self.WORLD_EDGES:
            raise ValueError(f"world_edges must be None or one of {self.WORLD_EDGES}, got {mode!r}")
        if world and mode is None:
            raise ValueError("the resident rollout of a feed built with world_pos= needs Rollout(..., world_edges="
                             '"frame" | "prediction" | "off"): without it the frames would be read in frame layout, '
                             "without the obstacle displacement columns the model was trained on")
        if not world:
            if mode is not None:
                raise ValueError(f"world_edges={mode!r} needs a feed built with world_pos=")
            return False
        if getattr(feed, "dynamic", False):
            # a dynamic_edges= feed: the topology is rebuilt every step, from the clean frame or from the x the
            # model sees; there is no static adjacency to fall back to
            if mode == "off":
                raise ValueError('world_edges="off" does not go with a feed built with dynamic_edges=: its world '
                                 'edges are rebuilt every step, from "frame" or from "prediction"')
        elif mode != "off" and feed.senders is None:
            raise ValueError(f"world_edges={mode!r} needs a feed whose world_pos= has an edge_index and an "
                             'edge_attr_start; use "off" for a model without edge_attr')
        if self.k != feed.node_type_index + 3:
            raise ValueError(f"node_type_index {self.k} differs from the feed's node_type_index + 3 = "
                             f"{feed.node_type_index + 3} (the batch layout of a world_pos= feed)")
        return True

    # ------------------------------------------------------------------ trajectory bookkeeping
    def reset(self):
        """Start a new trajectory (reference _reset_validation_trajectory)."""
        self.last_prediction = None
        self.last_previous = None

    def clear(self):
        """Forget recorded steps (reference _reset_validation_epoch_end)."""
        self.outputs.clear()
        self.targets.clear()
        self.losses.clear()
        self._res_sq, self._res_count = [], 0
        self.reset()

    # ------------------------------------------------------------------ one step
    def _predict(self, fr, last, last_prev):
        if last is not None:
            fr.x[:, self.os:self.oe] = last
            if self.use_prev:
                fr.x[:, self.ps:self.pe] = last_prev
        mask = build_mask(self.k, fr)
        current = fr.x[:, self.os:self.oe].clone()
        with torch.no_grad():
            _, _, pred = self.sim(fr)
        pred = torch.where(mask[:, None], fr.y, pred)
        prev = pred - current if self.use_prev else None
        return pred, prev

    def _eager(self, batch):
        fr = _Frame(x=batch.x.clone(), y=batch.y, edge_index=batch.edge_index, edge_attr=batch.edge_attr,
                    pos=getattr(batch, "pos", None))
        return self._predict(fr, self.last_prediction, self.last_previous)

    def _record(self, batch):
        dev = batch.x.device
        self._sx, self._sy = batch.x.clone(), batch.y.clone()
        self._sea = batch.edge_attr.clone() if batch.edge_attr is not None else None  # transformer models: none
        self._sei = batch.edge_index
        self._last = self.last_prediction.clone()
        self._lastp = self.last_previous.clone() if self.use_prev else None
        fr = _Frame(x=self._sx, y=self._sy, edge_index=self._sei, edge_attr=self._sea, pos=getattr(batch, "pos", None))
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):  # warm-up: topology cache, weight packs, allocator
            self._predict(fr, self._last, self._lastp)
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        # the graph reads this topology's buffers: keep them alive beyond the topology cache
        from graphphysics.models import _engine

        self._topo = _engine.get_topology(self._sei, self._sx.size(0))
        self._sx.copy_(batch.x)
        g = torch.cuda.CUDAGraph()
        import torch.distributed as dist

        # a process group's watchdog thread queries events while this thread records (see TrainStep)
        mode = "thread_local" if dist.is_available() and dist.is_initialized() else "global"
        with torch.cuda.graph(g, capture_error_mode=mode):
            pred, prev = self._predict(fr, self._last, self._lastp)
            self._last.copy_(pred)
            if self.use_prev:
                self._lastp.copy_(prev)
        self._graph, self._gpred, self._gprev = g, pred, prev
        self._key = (weakref.ref(batch.edge_index), batch.edge_index._version, batch.x.shape)

    def _same_mesh(self, batch):
        """The recorded graph holds the topology of this exact edge_index tensor (identity + version,
        as graphphysics.models._engine.get_topology) and static buffers of this x shape."""
        if self._key is None:
            return False
        ref, ver, shape = self._key
        return ref() is batch.edge_index and ver == batch.edge_index._version and shape == batch.x.shape

    def step(self, batch):
        """One _make_prediction on `batch` (x, y, edge_index, edge_attr on the device). Returns
        (predicted_outputs, target) and records them and the step's masked L2 loss."""
        if not self.use_graph or self.last_prediction is None:
            pred, prev = self._eager(batch)
        else:
            if self._graph is None or not self._same_mesh(batch):
                self._record(batch)
            else:
                self._sx.copy_(batch.x)
                self._sy.copy_(batch.y)
                if self._sea is not None:
                    self._sea.copy_(batch.edge_attr)
                self._last.copy_(self.last_prediction)
                if self.use_prev:
                    self._lastp.copy_(self.last_previous)
            self._graph.replay()
            pred = self._gpred.clone()
            prev = self._gprev.clone() if self.use_prev else None
        self.last_prediction, self.last_previous = pred, prev
        node_type = batch.x[:, self.k]
        self.outputs.append(pred)
        self.targets.append(batch.y)
        self.losses.append(masked_mse(batch.y, pred, node_type, self.masks))
        return pred, batch.y

    def rollout(self, frames):
        """Run a whole trajectory (iterable of batches); returns the stacked predictions."""
        self.reset()
        return torch.stack([self.step(b)[0] for b in frames])

    # ------------------------------------------------------------------ resident trajectories
    def _resident_same(self, batch, keep):
        """As _same_mesh: the state (and its recorded graph) holds the topology of this exact edge_index tensor
        and buffers of these shapes; keeping the predictions or not is part of what was recorded."""
        if self._res is None:
            return False
        ref, ver, xs, ys, ea, kept, mode, acc = self._res.key
        return (ref() is batch.edge_index and ver == batch.edge_index._version and xs == batch.x.shape
                and ys == batch.y.shape and ea == (None if batch.edge_attr is None else batch.edge_attr.shape)
                and kept == keep and mode == self.world_edges and acc == self.acceleration)

    def _resident_alloc(self, batch, keep):
        feed, dev = self.feed, batch.x.device
        d, cap = self.oe - self.os, self.feed.T - 1  # a trajectory of T frames has at most T − 1 steps
        st = _Resident()
        st.x, st.y = batch.x.clone(), batch.y.clone()
        st.edge_attr = batch.edge_attr.clone() if batch.edge_attr is not None else None  # transformer models: none
        st.frame = _Frame(x=st.x, y=st.y, edge_index=batch.edge_index, edge_attr=st.edge_attr,
                          pos=getattr(batch, "pos", None))
        st.last = torch.zeros(feed.N, d, dtype=torch.float32, device=dev)
        st.last_prev = torch.zeros_like(st.last) if self.use_prev else None
        st.preds = torch.zeros(cap, feed.N, d, dtype=torch.float32, device=dev) if keep else None
        st.loss = torch.zeros(cap, dtype=torch.float32, device=dev)
        st.sq = torch.zeros(cap, dtype=torch.float32, device=dev)
        st.cursor = torch.zeros(1, dtype=torch.int32, device=dev)  # the step counter: only the end stage writes it
        st.obstacle_mean, st.world_clean = None, None
        if self.world_edges is not None:  # a world_pos= feed (checked by the caller)
            st.obstacle_mean = torch.zeros(feed.B, 3, dtype=torch.float32, device=dev)
            if self.world_edges == "frame":  # the clean world positions of the step's frame: the edges' input
                st.world_clean = torch.zeros(feed.N, 3, dtype=torch.float32, device=dev)
        st.num_edges = None
        if getattr(feed, "dynamic", False):  # the edge count of every step's rebuilt topology
            st.num_edges = torch.zeros(cap, dtype=torch.int32, device=dev)
        st.ws, st.graph, st.topo = None, None, None
        if dev.type == "cuda":
            from graphphysics import _native as nat

            st.ws = nat.rollout_end_workspace(feed.N, dev)
        st.key = (weakref.ref(batch.edge_index), batch.edge_index._version, batch.x.shape, batch.y.shape,
                  None if batch.edge_attr is None else batch.edge_attr.shape, keep, self.world_edges,
                  self.acceleration)
        return st

    def _resident_step(self, st):
        """Step `cursor`: frame and feedback into the static batch, the evaluation forward, mask / state /
        results. Three stages of device work and nothing else, so it records as it runs."""
        feed, mode = self.feed, self.world_edges
        if st.x.is_cuda:
            from graphphysics import _native as nat

            begin, end, extra = nat.rollout_begin, nat.rollout_end, (st.ws,)
            begin_world, begin_aneurysm = nat.rollout_begin_world, nat.rollout_begin_aneurysm
        else:
            from graphphysics.dataset.resident import rollout_begin_torch as begin, rollout_end_torch as end
            from graphphysics.dataset.resident import rollout_begin_world_torch as begin_world
            from graphphysics.dataset.resident import rollout_begin_aneurysm_torch as begin_aneurysm

            extra = ()
        if self.acceleration is not None:  # an aneurysm= feed: both modes differ only in the previous-data columns
            begin_aneurysm(feed.traj, feed.graph_ptr, feed.frame, st.cursor, feed.y_columns, feed.pos, feed.node_type,
                           feed.inflow_stats, (self.os, self.oe), self._prev_cols, st.last, st.last_prev, st.x, st.y)
        elif mode is None:
            begin(feed.traj, feed.graph_ptr, feed.frame, st.cursor, feed.y_columns, (self.os, self.oe),
                  self._prev_cols, st.last, st.last_prev, st.x, st.y)
        else:
            begin_world(feed.traj, feed.graph_ptr, feed.frame, st.cursor, feed.y_columns, feed.node_type_index,
                        (self.os, self.oe), self._prev_cols, st.last, st.last_prev, st.x, st.y, st.obstacle_mean,
                        st.world_clean)
            if getattr(feed, "dynamic", False):
                # add_world_edges on the step's positions, between the begin stage and the forward: the bound
                # topology is rewritten in place, st.frame.edge_index is its handle (on the CPU: the live columns)
                feed.build_edges(st.world_clean if mode == "frame" else st.x, st.x[:, self.k])
                st.num_edges.index_copy_(0, st.cursor.to(torch.int64), feed.num_edges_dev)
                if not st.x.is_cuda:
                    st.frame.edge_index = feed.current_edge_index()
            elif mode != "off":  # "frame": the clean positions of the frame; "prediction": what the model sees
                pos = st.world_clean if mode == "frame" else st.x
                if st.x.is_cuda:
                    nat.feed_world_edge_features(feed.senders, feed.receivers, pos, st.edge_attr,
                                                 feed.edge_attr_start)
                else:
                    from graphphysics.dataset.resident import world_edge_features_torch

                    world_edge_features_torch(pos, feed._world_edge_index, st.edge_attr, feed.edge_attr_start)
        with torch.no_grad():
            _, _, out = self.sim(st.frame)
        end(out, st.y, st.x, self.k, self.masks, self.os, st.last, st.last_prev, st.preds, st.cursor, st.loss, st.sq,
            *extra)

    def _resident_record(self, st):
        dev = st.x.device
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):  # warm-up: topology cache, weight packs, allocator
            st.cursor.zero_()
            self._resident_step(st)
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        # the graph reads this topology's buffers: keep them alive beyond the topology cache
        from graphphysics.models import _engine

        st.topo = _engine.get_topology(st.frame.edge_index, st.x.size(0))
        g = torch.cuda.CUDAGraph()
        import torch.distributed as dist

        mode = "thread_local" if dist.is_available() and dist.is_initialized() else "global"  # see _record
        with torch.cuda.graph(g, capture_error_mode=mode):
            self._resident_step(st)
        st.graph = g
        self.resident_records += 1

    def rollout_resident(self, batch, start=0, steps=None, keep_predictions=True):
        """One whole trajectory from the feed's resident frames: step s reads frame start[g] + s of graph g,
        feeds the previous prediction back from step 1 on, and compares with frame start[g] + s + 1 — _predict
        and step over `steps` frames, with the step counter, the feedback state and the results on the device.
        With graph=True (HIP tensors) every step is one replay of one captured graph, recorded on the first call
        and again only when the mesh (edge_index) or the shapes change; otherwise, and on CPU tensors (torch
        forms), the same three stages run eagerly per step.

        batch: the static x [N, >= F], y [N, d], edge_index, edge_attr (None for transformer models) and pos;
        cloned like TrainStep's (x's columns beyond F and edge_attr are re-read on every call). With a world_pos=
        feed (world_edges=, module docstring) x is [N, >= F + 3] and, unless the mode is "off", edge_attr is
        [E, >= edge_attr_start + 4]: the step rewrites those four columns of its own copy, never the caller's. With an
        aneurysm= feed (acceleration=, module docstring) x is [N, >= F + 10] and every start lies in [1, T − 2]. start:
        an int or one int per graph; steps: default T − 1 − max(start). Returns the predictions [steps, N, d] (None
        with keep_predictions=False); extends self.losses by the per-step losses (0-dim device tensors) and
        adds to what all_rollout_rmse() reports. Nothing here synchronises with the host."""
        feed = self.feed
        if feed is None:
            raise ValueError("rollout_resident needs Rollout(..., feed=ResidentTrajectories)")
        world = self._check_world(feed)
        self._check_acceleration(feed)
        if self.sim.training:
            raise RuntimeError("rollout_resident runs the evaluation forward: call sim.eval() first")
        x, y, d = batch.x, batch.y, self.oe - self.os
        if x.device != feed.traj.device or x.dtype != torch.float32 or x.dim() != 2 or x.shape[0] != feed.N or \
                x.shape[1] < feed.Fx or self.k >= x.shape[1]:
            raise ValueError(f"batch.x must be fp32 [{feed.N}, >= {max(feed.Fx, self.k + 1)}] on {feed.traj.device}, "
                             f"got {tuple(x.shape)} {x.dtype} on {x.device}")
        if y is None or y.device != x.device or y.dtype != torch.float32 or tuple(y.shape) != (feed.N, d):
            raise ValueError(f"batch.y must be fp32 [{feed.N}, {d}] on {feed.traj.device}")
        dynamic = world and getattr(feed, "dynamic", False)
        if dynamic and batch.edge_index is not feed.edge_index:
            raise ValueError("with a dynamic_edges= feed, batch.edge_index must be the feed's own edge_index tensor "
                             "(feed.edge_index): it is the handle of the topology the steps rebuild")
        if world and self.world_edges != "off" and not dynamic:
            ea, E, A = getattr(batch, "edge_attr", None), feed.senders.numel(), feed.edge_attr_start + 4
            if ea is None or ea.device != x.device or ea.dtype != torch.float32 or ea.dim() != 2 or \
                    ea.shape[0] != E or ea.shape[1] < A or ea.stride(1) != 1:
                raise ValueError(f"batch.edge_attr must be fp32 [{E}, >= {A}] on {feed.traj.device} with unit column "
                                 "stride")
        if torch.is_tensor(start):
            start = start.tolist()
        starts = [int(s) for s in start] if isinstance(start, (list, tuple)) else [int(start)] * feed.B
        if len(starts) != feed.B:
            raise ValueError(f"expected one start frame per graph ({feed.B}), got {len(starts)}")
        steps = feed.T - 1 - max(starts) if steps is None else int(steps)
        if steps < 1 or max(starts) + steps > feed.T - 1:
            raise ValueError(f"start {starts} and {steps} steps leave the trajectory: step s reads frames "
                             f"start + s and start + s + 1 of {feed.T}")
        feed.set_frames(starts)  # the host check of every start frame; the feed is in explicit mode from here
        keep = bool(keep_predictions)
        if self._resident_same(batch, keep):
            st = self._res
            st.x.copy_(x)
            if st.edge_attr is not None:
                st.edge_attr.copy_(batch.edge_attr)
        else:
            st = self._res = self._resident_alloc(batch, keep)
        if steps > st.loss.numel():
            raise ValueError(f"{steps} steps exceed the result buffers' capacity {st.loss.numel()}")
        captured = self.use_graph and x.is_cuda
        if captured and st.graph is None:
            self._resident_record(st)
        st.cursor.zero_()  # every call is a new trajectory; `last` is not read at step 0
        for _ in range(steps):
            if captured:
                st.graph.replay()
            else:
                self._resident_step(st)
        # a dynamic_edges= feed: the edge count of every step's topology (device int32 [steps]); None otherwise
        self.resident_num_edges = st.num_edges[:steps].clone() if st.num_edges is not None else None
        loss, sq = st.loss[:steps].clone(), st.sq[:steps].clone()
        self.losses.extend(loss.unbind(0))
        self._res_sq.append(sq)
        self._res_count += steps * feed.N * d
        return st.preds[:steps].clone() if keep else None

    def all_rollout_rmse(self):
        if not self._res_sq:
            p = torch.cat([o.float() for o in self.outputs])
            t = torch.cat([o.float() for o in self.targets])
            return math.sqrt(((p - t) ** 2).mean().item())
        # resident runs keep Σ (pred − target)² per step on the device: add them, in fp64 on the host, to what
        # the lists hold
        total, count = float(torch.cat(self._res_sq).cpu().double().sum()), self._res_count
        for o, t in zip(self.outputs, self.targets):
            total += float(((o.float() - t.float()) ** 2).sum().double())
            count += o.numel()
        return math.sqrt(total / count)
