"""Drop-in for the `libply_c` functions of the reference that run on the GPU here (partition/partition.py:124-150:
`libply_c.prune`, `libply_c.compute_geof`; supervized_partition/losses.py:134 and graph_processing.py: `libply_c.connected_comp`);
see graphs.py and ops.connected_components."""
import numpy as np
import torch

from .. import ops
from .graphs import _dev, compute_geof, prune  # noqa: F401


def connected_comp(n_ver, source, target, active, cutoff):
    """connected components of the graph restricted to its active edges (reference partition/ply_c/ply_c.cpp connected_comp,
    called with cutoff 0) -> (components: list of ascending vertex index arrays, in_component uint32 [n_ver]); components are
    numbered by their smallest vertex.  cutoff > 0 (merging components smaller than cutoff) is not supported."""
    if cutoff > 0:
        raise NotImplementedError('connected_comp: cutoff > 0 (the merge of small components) is not supported on the device')
    dev = _dev()
    up = lambda a, t: ops.upload(torch.from_numpy(np.ascontiguousarray(a).reshape(-1).astype(t, copy=False)), dev)
    g = ops.EdgeGraph(up(source, np.int64), up(target, np.int64), int(n_ver))
    comp, k, _ = ops.connected_components(g, up(np.asarray(active) != 0, np.uint8))
    in_component = comp.cpu().numpy().astype(np.uint32)
    order = np.argsort(in_component, kind='stable')
    bounds = np.searchsorted(in_component[order], np.arange(k + 1))
    components = [order[bounds[i]:bounds[i + 1]] for i in range(k)]
    return components, in_component
