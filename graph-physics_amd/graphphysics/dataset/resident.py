"""Training batches from trajectories that stay resident, and clean, on the device.

What the reference does per item in Dataset.__getitem__ — x is frame t of a trajectory, y the dynamic
columns of frame t + 1 (reference dataset/h5_dataset.py:81-92, dataset/hierarchical.py:96-116), then
add_noise on the noisy columns of NORMAL nodes (dataset/preprocessing.py:177-238) — as ONE libmgn launch
(mgn_feed_batch) that writes a batch's x and y in place from per-graph frame indices. The frame indices
(torch.randint) and the Gaussian draws (torch.randn) are device work too, so ResidentTrajectories.fill can be
recorded at the head of a captured training step (TrainStep(..., feed=...)) and draws anew on every replay.

The stored frames are only ever read: the in-place write of preprocessing.add_noise, applied to frames kept
on the device, would pile noise on noise epoch after epoch (the reference re-reads every item from disk and
never sees this); here the noise goes into the batch, never into `traj`.

Not supported: `previous_data`, per-frame positions or edge_attr (Lagrangian datasets), and trajectories of
unequal length in one batch. batch.edge_index / edge_attr are never touched.

The validation rollout reads the same resident frames (training.rollout.Rollout.rollout_resident):
rollout_begin_torch / rollout_end_torch state, as torch ops on any device, the two rules libmgn's
mgn_rollout_begin / mgn_rollout_end run around the Simulator's evaluation forward; there previous data is
supported, noise is not applied.
"""
import math

import torch

from graphphysics import _native as nat
from graphphysics.utils.nodetype import NodeType


def _noise_lists(noise):
    """(starts, ends, scales) of the reference's noise_parameters, with add_noise's checks and messages."""
    start, end, scale = noise["noise_index_start"], noise["noise_index_end"], noise["noise_scale"]
    if isinstance(start, int):
        start = [start]
    if isinstance(end, int):
        end = [end]
    if isinstance(scale, (int, float)):
        scale = [float(scale)] * len(start)
    if len(start) != len(end):
        raise ValueError("noise_index_start and noise_index_end must have the same length.")
    if len(scale) != len(start):
        raise ValueError("noise_scale must have the same length as noise_index_start and noise_index_end.")
    return [int(s) for s in start], [int(e) for e in end], [float(s) for s in scale]


def _check_ranges(ranges, F):
    if len(ranges) > nat.MGN_FEED_MAX_RANGES:
        raise ValueError(f"at most {nat.MGN_FEED_MAX_RANGES} noisy column ranges are supported, got {len(ranges)}")
    for i, (s, e) in enumerate(ranges):
        if not 0 <= s <= e <= F:
            raise ValueError(f"noisy column range ({s}, {e}) is outside [0, {F}]")
        for s2, e2 in ranges[:i]:
            if s < e and s2 < e2 and s < e2 and s2 < e:
                raise ValueError(f"noisy column ranges ({s2}, {e2}) and ({s}, {e}) overlap")


def _node_graph(graph_ptr, N, device):
    """Graph id of every node from node offsets [B+1] (a host list or a tensor)."""
    gp = torch.as_tensor(graph_ptr, dtype=torch.int64).to(device)
    return torch.repeat_interleave(torch.arange(gp.numel() - 1, device=device), gp[1:] - gp[:-1], output_size=N)


def fill_torch(traj, graph_ptr, frame, y_columns, node_type_index, ranges, scales, z):
    """mgn_feed_batch's rule as torch ops on any device: returns (x [N, F], y [N, y_end - y_start]) as new
    tensors. x = frame[g] of traj for the nodes of graph g, plus z[:, zc] * scales[i] on the columns of
    noisy range i of the rows whose (clean) node type is NORMAL — zc runs over the ranges in order; y = the
    y_columns of the next clean frame. z None: no noise. What ResidentTrajectories.fill runs on CPU tensors,
    and what the kernel is tested and timed against."""
    T, N, F = traj.shape
    rows = torch.arange(N, device=traj.device)
    t = frame.to(traj.device, torch.int64)[_node_graph(graph_ptr, N, traj.device)]
    x = traj[t, rows]
    y = traj[t + 1, rows, y_columns[0]:y_columns[1]].contiguous()
    if z is not None:
        normal = (x[:, node_type_index] == NodeType.NORMAL)[:, None]
        zc = 0
        for i, (s, e) in enumerate(ranges):
            feature = x[:, s:e]
            noise = z[:, zc:zc + e - s] * scales[i]
            x[:, s:e] = torch.where(normal, feature + noise, feature)
            zc += e - s
    return x, y


def check_rollout_columns(F, y_columns, out_columns, prev_columns, node_type_index):
    """The host-side preconditions of a resident rollout (ValueError): the model's output columns, the target
    columns and, when used, the previous-data columns have one width d; the output and previous-data ranges
    lie inside [0, F), do not overlap, and do not contain the node-type column (the rollout writes them,
    and reads the node type of the written row). Returns d."""
    (ys, ye), (os_, oe) = (int(v) for v in y_columns), (int(v) for v in out_columns)
    d = oe - os_
    if d < 1 or not 0 <= os_ < oe <= F:
        raise ValueError(f"output columns ({os_}, {oe}) must be a non-empty range inside [0, {F})")
    if ye - ys != d:
        raise ValueError(f"the feed's y_columns ({ys}, {ye}) and the output columns ({os_}, {oe}) differ in width")
    k = int(node_type_index)
    if os_ <= k < oe:
        raise ValueError(f"node_type_index {k} lies inside the output columns ({os_}, {oe})")
    if prev_columns is not None:
        ps, pe = (int(v) for v in prev_columns)
        if not 0 <= ps < pe <= F:
            raise ValueError(f"previous-data columns ({ps}, {pe}) must be a non-empty range inside [0, {F})")
        if pe - ps != d:
            raise ValueError(f"previous-data columns ({ps}, {pe}) and the output columns ({os_}, {oe}) differ in width")
        if ps < oe and os_ < pe:
            raise ValueError(f"previous-data columns ({ps}, {pe}) overlap the output columns ({os_}, {oe})")
        if ps <= k < pe:
            raise ValueError(f"node_type_index {k} lies inside the previous-data columns ({ps}, {pe})")
    return d


def rollout_begin_torch(traj, graph_ptr, frame, cursor, y_columns, out_columns, prev_columns, last, last_prev, x, y):
    """mgn_rollout_begin's rule as torch ops on any device, in place on x [N, >= F] and y [N, d]: with
    s = cursor (a one-element int tensor or an int) x[:, :F] = frame[g] + s of traj for the nodes of graph g,
    then, when s > 0, x[:, out_columns] = last and x[:, prev_columns] = last_prev (prev_columns None: no
    previous data); y = y_columns of the following frame. traj is only read. The CPU path of
    Rollout.rollout_resident, and what the kernel is tested and timed against."""
    T, N, F = traj.shape
    s = int(cursor)
    rows = torch.arange(N, device=traj.device)
    t = frame.to(traj.device, torch.int64)[_node_graph(graph_ptr, N, traj.device)] + s
    x[:, :F] = traj[t, rows]
    if s > 0:
        x[:, out_columns[0]:out_columns[1]] = last
        if prev_columns is not None and prev_columns[1] > prev_columns[0]:
            x[:, prev_columns[0]:prev_columns[1]] = last_prev
    y.copy_(traj[t + 1, rows, y_columns[0]:y_columns[1]])


def rollout_end_torch(out, y, x, node_type_index, masks, out_start, last, last_prev, preds, cursor, loss, sq):
    """mgn_rollout_end's rule as torch ops on any device, in place on its state: with s = cursor,
    pred = y where the node type x[:, node_type_index] is neither NORMAL nor OUTFLOW (training.rollout.build_mask)
    and out elsewhere; last_prev = pred - x[:, out columns] (None: not kept), last = pred, preds[s] = pred (None:
    not kept), loss[s] = masked_mse(y, pred, node type, masks) — masked_mse itself —, sq[s] = Σ (pred - y)²,
    cursor += 1 (cursor: a one-element int tensor). Returns pred."""
    from graphphysics.utils.loss import masked_mse

    s = int(cursor)
    d = out.shape[1]
    node_type = x[:, node_type_index]
    keep = torch.logical_not(torch.logical_or(node_type == NodeType.NORMAL, node_type == NodeType.OUTFLOW))
    pred = torch.where(keep[:, None], y, out)
    if last_prev is not None:
        last_prev.copy_(pred - x[:, out_start:out_start + d])
    last.copy_(pred)
    if preds is not None:
        preds[s] = pred
    loss[s] = masked_mse(y, pred, node_type, list(masks))
    sq[s] = ((pred - y) ** 2).sum()
    cursor += 1
    return pred


class ResidentTrajectories:
    """traj: fp32 [T, N, F] on the device, N the nodes of the batch's graphs concatenated (as
    meshes.cylinder_batch lays them out), every graph with the same T frames. graph_ptr: [B+1] node offsets
    (host list or tensor; validated). y_columns = (start, end): the columns of the next frame that are the
    target. noise: the reference's noise_parameters dict (noise_index_start / noise_index_end / noise_scale
    as an int, a float or lists; its node_type_index must equal node_type_index) or None. frames: "random"
    (every fill draws one frame per graph, uniform over the frames that have a successor) or explicit
    per-graph frames (see set_frames).

    frame [B] int32, z [N, W] fp32 (None without noise) and scales [n] fp32 (None without noise) are
    allocated once and only rewritten: a captured graph keeps reading the same addresses, tests and users
    read there what the last fill used. Not supported: previous_data, per-frame positions or edge_attr,
    trajectories of unequal length (module docstring)."""

    def __init__(self, traj, graph_ptr, y_columns, node_type_index, noise=None, frames="random"):
        if not torch.is_tensor(traj) or traj.dtype != torch.float32 or traj.dim() != 3 or not traj.is_contiguous():
            raise ValueError("traj must be a contiguous fp32 [T, N, F] tensor")
        T, N, F = traj.shape
        if T < 2:
            raise ValueError("traj needs at least 2 frames: x is frame t, y comes from frame t + 1")
        gp = [int(v) for v in (graph_ptr.tolist() if torch.is_tensor(graph_ptr) else graph_ptr)]
        if len(gp) < 2 or gp[0] != 0 or gp[-1] != N or any(b < a for a, b in zip(gp, gp[1:])):
            raise ValueError(f"graph_ptr must hold B + 1 non-decreasing node offsets from 0 to N = {N}, got {gp}")
        ys, ye = int(y_columns[0]), int(y_columns[1])
        if not 0 <= ys < ye <= F:
            raise ValueError(f"y_columns ({ys}, {ye}) must be a non-empty range inside [0, {F}]")
        if not 0 <= int(node_type_index) < F:
            raise ValueError(f"node_type_index {node_type_index} is outside [0, {F})")
        self.traj, self.T, self.N, self.F, self.B = traj, T, N, F, len(gp) - 1
        self.y_columns, self.node_type_index = (ys, ye), int(node_type_index)
        dev = traj.device
        self.graph_ptr = torch.tensor(gp, dtype=torch.int32, device=dev)
        self.ranges, self._base_scales, self.scales, self.z = [], [], None, None
        if noise is not None:
            if int(noise["node_type_index"]) != self.node_type_index:
                raise ValueError(f"noise node_type_index {noise['node_type_index']} differs from node_type_index "
                                 f"{self.node_type_index}")
            start, end, self._base_scales = _noise_lists(noise)
            self.ranges = list(zip(start, end))
            _check_ranges(self.ranges, F)
            width = sum(e - s for s, e in self.ranges)
            if width > 0:
                self.scales = torch.tensor(self._base_scales, dtype=torch.float32, device=dev)
                self.z = torch.zeros(N, width, dtype=torch.float32, device=dev)
        self._ranges_c = nat.feed_ranges(self.ranges)
        self.frame = torch.zeros(self.B, dtype=torch.int32, device=dev)
        self.random_frames = True
        self.set_frames(frames)

    def set_frames(self, frames):
        """"random": every fill draws its frames. A host list / CPU tensor of B frames, each in [0, T-2]
        (ValueError otherwise): the fills use these until the next set_frames."""
        if isinstance(frames, str):
            if frames != "random":
                raise ValueError(f'frames must be "random" or B = {self.B} frame indices, got {frames!r}')
            self.random_frames = True
            return
        fr = [int(f) for f in (frames.tolist() if torch.is_tensor(frames) else frames)]
        if len(fr) != self.B:
            raise ValueError(f"expected one frame per graph ({self.B}), got {len(fr)}")
        if any(f < 0 or f > self.T - 2 for f in fr):
            raise ValueError(f"frames must lie in [0, {self.T - 2}] (frame t needs its successor t + 1), got {fr}")
        self.random_frames = False
        self.frame.copy_(torch.tensor(fr, dtype=torch.int32))

    def set_noise_t(self, t):
        """The reference's noise curriculum: scale_i = 10 · scale_i · (1 + cos(t π)); None: the plain scales.
        Rewrites the persistent scales tensor (a captured graph reads it at replay: no re-capture)."""
        if self.scales is None:
            return
        s = self._base_scales if t is None else [10 * b * (1 + math.cos(t * math.pi)) for b in self._base_scales]
        self.scales.copy_(torch.tensor(s, dtype=torch.float32))

    def fill(self, batch):
        """Write batch.x[:, :F] and batch.y in place: device work only, capturable. HIP tensors: the frame /
        noise draws and one mgn_feed_batch launch (no fallback); CPU tensors: fill_torch."""
        x, y = batch.x, batch.y
        if x.device != self.traj.device or x.dtype != torch.float32 or x.dim() != 2 or x.shape[0] != self.N or \
                x.shape[1] < self.F:
            raise ValueError(f"batch.x must be fp32 [{self.N}, >= {self.F}] on {self.traj.device}, got "
                             f"{tuple(x.shape)} {x.dtype} on {x.device}")
        wy = self.y_columns[1] - self.y_columns[0]
        if y is None or y.device != x.device or y.dtype != torch.float32 or tuple(y.shape) != (self.N, wy):
            raise ValueError(f"batch.y must be fp32 [{self.N}, {wy}] on {self.traj.device}")
        with torch.no_grad():
            if self.random_frames:
                self.frame.random_(0, self.T - 1)  # torch.randint(0, T-1, (B,)) into the persistent tensor
            if self.z is not None:
                self.z.normal_()
            if self.traj.is_cuda:
                nat.feed_batch(self.traj, self.graph_ptr, self.frame, self.y_columns, self.node_type_index,
                               self._ranges_c, self.scales, self.z, x, y)
            else:
                fx, fy = fill_torch(self.traj, self.graph_ptr, self.frame, self.y_columns, self.node_type_index,
                                    self.ranges, self.scales, self.z)
                x[:, :self.F] = fx
                y.copy_(fy)
        return batch
