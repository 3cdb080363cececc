"""Drop-in graph preprocessing (reference graphphysics/dataset/preprocessing.py) on the device.

Same function names, arguments and Data-in/Data-out contract as the reference; the index work
(FaceToEdge, to_undirected, radius search, edge features) runs in libmgn on the graph's HIP
device (graphphysics.utils.graph_build), the O(N) feature edits as device torch ops.

  add_edge_features        preprocessing.py:16-23
  add_obstacles_next_pos   preprocessing.py:49-89
  add_world_edges          preprocessing.py:92-140  (cKDTree.query_pairs → grid radius search)
  add_world_pos_features   preprocessing.py:143-174
  add_noise                preprocessing.py:177-238
  Random3DRotate           preprocessing.py:277-366 (one random rotation of pos, triples of x, and y)
  build_preprocessing      preprocessing.py:369-440 (noise, world-pos and edge-feature stages)

Random3DRotate is the per-item transform, for a host-side pipeline (an entry of extra_node_features). Inside a
captured training step the same augmentation is drawn and applied on the device by the resident feed:
dataset.resident.ResidentTrajectories(..., rotate=...).

compute_min_distance_to_type (a one-off aneurysm feature builder, not per-step work) is outside the MGN hot
path and is not provided.
"""
import copy
import math
import random
from functools import partial
from typing import Callable, List, Optional, Tuple, Union

import torch

from graphphysics import transforms as T
from graphphysics.utils import graph_build as G
from graphphysics.utils.nodetype import NodeType


def add_edge_features() -> List[Callable]:
    return [T.Cartesian(norm=False), T.Distance(norm=False)]


def _3d_face_to_edge(graph):
    """Quad faces [4, F] → the four triangles the reference forms (preprocessing.py:26-46)."""
    face = graph.face
    graph.face = torch.cat([face[0:3], face[1:4], torch.stack([face[2], face[3], face[0]], dim=0),
                            torch.stack([face[3], face[0], face[1]], dim=0)], dim=1)
    return graph


def add_obstacles_next_pos(graph, world_pos_index_start: int, world_pos_index_end: int, node_type_index: int):
    world_pos = graph.x[:, world_pos_index_start:world_pos_index_end]
    other = graph.x[:, world_pos_index_end:]
    disp = graph.y[:, world_pos_index_start:world_pos_index_end] - world_pos
    # node_type_index refers to the layout after the 3 displacement columns are inserted
    node_type = graph.x[:, node_type_index - 3]
    obst = node_type == NodeType.OBSTACLE
    mean_disp = torch.mean(disp[obst], dim=0)
    disp[~obst] = mean_disp
    graph.x = torch.cat([world_pos, disp, other], dim=1)
    return graph


def add_world_edges(graph, world_pos_index_start: int, world_pos_index_end: int, node_type_index: int,
                    radius: float = 0.03):
    world_pos = graph.x[:, world_pos_index_start:world_pos_index_end]
    added = G.radius_pairs(world_pos, radius, node_type=graph.x[:, node_type_index])
    edge_index = torch.cat([added, graph.edge_index.to(added.dtype)], dim=1)
    graph.edge_index = G.to_undirected(edge_index, graph.x.size(0))
    return graph


def add_world_pos_features(graph, world_pos_index_start: int, world_pos_index_end: int):
    f = G.edge_features(graph.x[:, world_pos_index_start:world_pos_index_end], graph.edge_index)
    graph.edge_attr = torch.cat([graph.edge_attr, f.type_as(graph.edge_attr)], dim=-1)
    return graph


def add_noise(graph, noise_index_start: Union[int, List[int]], noise_index_end: Union[int, List[int]],
              noise_scale: Union[float, List[float]], node_type_index: int, t: Optional[float] = None):
    """The reference's add_noise, its in-place write of graph.x included: on frames that are kept on the device
    and reused (rather than re-read per item, as the reference's datasets do) the noise accumulates in the stored
    data call after call — pass a copy, or train from dataset.resident.ResidentTrajectories, which never writes
    the stored frames."""
    if isinstance(noise_index_start, int):
        noise_index_start = [noise_index_start]
    if isinstance(noise_index_end, int):
        noise_index_end = [noise_index_end]
    if isinstance(noise_scale, float):
        noise_scale = [noise_scale] * len(noise_index_start)
    if len(noise_index_start) != len(noise_index_end):
        raise ValueError("noise_index_start and noise_index_end must have the same length.")
    if len(noise_scale) != len(noise_index_start):
        raise ValueError("noise_scale must have the same length as noise_index_start and noise_index_end.")
    mask = graph.x[:, node_type_index] != NodeType.NORMAL
    for start, end, scale in zip(noise_index_start, noise_index_end, noise_scale):
        feature = graph.x[:, start:end]
        s = 10 * scale * (1 + math.cos(t * math.pi)) if t is not None else scale
        noise = torch.randn_like(feature) * s
        noise[mask] = 0
        graph.x[:, start:end] = feature + noise
    return graph


class Random3DRotate:
    """The reference's Random3DRotate: one random 3D rotation applied to the node positions, to the 3-column
    ranges `feature_indices` of graph.x, and to the first 3 columns of graph.y. Row vectors times the matrix
    (v @ R), torch ops on whatever device the tensors are on. As in the reference, x is written in place while
    pos and y are rebound to new tensors, and a y wider than 3 columns comes back 3 wide."""

    def __init__(self, feature_indices: List[Tuple[int, int]] = None) -> None:
        self.feature_indices = feature_indices or []
        for s, e in self.feature_indices:
            assert e - s == 3, f"a rotated feature range holds the 3 columns of one xyz vector, got ({s}, {e})"

    def _get_random_angles(self):
        """[alpha (about z), beta (about y), gamma (about x)] in radians: three draws of
        random.uniform(-180, 180) degrees, in that order."""
        return [math.radians(random.uniform(-180, 180)) for _ in range(3)]

    def _build_rotation_matrix(self, alpha, beta, gamma):
        """The reference's 3x3 matrix of yaw alpha, pitch beta and roll gamma (radians), computed in Python
        floats with its order of operations, as a torch tensor of the default dtype."""
        ca, sa = math.cos(alpha), math.sin(alpha)
        cb, sb = math.cos(beta), math.sin(beta)
        cg, sg = math.cos(gamma), math.sin(gamma)
        return torch.tensor([[ca * cb, ca * sb * sg + sa * cg, -ca * sb * cg + sa * sg],
                             [-sa * cb, -sa * sb * sg + ca * cg, sa * sb * cg + ca * sg],
                             [sb, -cb * sg, cb * cg]])

    def _rotate_features(self, x: torch.Tensor, matrix: torch.Tensor) -> torch.Tensor:
        """x with every range of feature_indices replaced by range @ matrix; written in place."""
        m = matrix.to(x.device, x.dtype)
        for s, e in self.feature_indices:
            x[:, s:e] = x[:, s:e] @ m
        return x

    def forward(self, data):
        R = self._build_rotation_matrix(*self._get_random_angles())
        pos = getattr(data, "pos", None)
        if pos is not None:
            pos = pos.view(-1, 1) if pos.dim() == 1 else pos
            assert pos.size(-1) == 3, "Node positions must be 3-dimensional"
            data.pos = pos @ R.to(pos.device, pos.dtype)
        if getattr(data, "x", None) is not None and self.feature_indices:
            data.x = self._rotate_features(data.x, R)
        if hasattr(data, "y") and data.x is not None:  # the reference's condition; only the first 3 columns stay
            y = data.y[:, 0:3]
            data.y = y @ R.to(y.device, y.dtype)
        return data

    def __call__(self, data):
        # torch_geometric's BaseTransform: forward on a shallow copy, so pos and y are rebound on the copy only
        return self.forward(copy.copy(data))

    def __repr__(self) -> str:
        return f"{self.__class__.__name__}({self.feature_indices})"


def build_preprocessing(noise_parameters: Optional[dict] = None, world_pos_parameters: Optional[dict] = None,
                        add_edges_features: bool = True,
                        extra_node_features: Optional[Union[Callable, List[Callable]]] = None,
                        extra_edge_features: Optional[Union[Callable, List[Callable]]] = None) -> T.Compose:
    pre: List[Callable] = []
    if extra_node_features is not None:
        pre.extend(extra_node_features if isinstance(extra_node_features, list) else [extra_node_features])
    if world_pos_parameters is not None:
        ws, we = world_pos_parameters["world_pos_index_start"], world_pos_parameters["world_pos_index_end"]
        nti = world_pos_parameters["node_type_index"]
        pre.extend([
            partial(add_obstacles_next_pos, world_pos_index_start=ws, world_pos_index_end=we, node_type_index=nti),
            T.FaceToEdge(remove_faces=False),
            partial(add_world_edges, world_pos_index_start=ws, world_pos_index_end=we, node_type_index=nti,
                    radius=world_pos_parameters.get("radius", 0.03)),
        ])
        pre.extend(add_edge_features())
        pre.append(partial(add_world_pos_features, world_pos_index_start=ws, world_pos_index_end=we))
    else:
        pre.append(T.FaceToEdge(remove_faces=False))
        if add_edges_features:
            pre.extend(add_edge_features())
    if noise_parameters is not None:
        # the reference inserts the noise stage after the first transform (preprocessing.py:433-442)
        pre.insert(1, partial(add_noise, noise_index_start=noise_parameters["noise_index_start"],
                           noise_index_end=noise_parameters["noise_index_end"],
                           noise_scale=noise_parameters["noise_scale"],
                           node_type_index=noise_parameters["node_type_index"]))
    if extra_edge_features is not None:
        pre.extend(extra_edge_features if isinstance(extra_edge_features, list) else [extra_edge_features])
    return T.Compose(pre)
