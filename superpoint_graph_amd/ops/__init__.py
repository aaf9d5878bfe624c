"""Tensor-level wrappers over the C ABI (include/spg_hip.h), one module per pipeline stage: torch owns device memory and streams, the
HIP library does the arithmetic.  model and batch serve the training step; spgraph, edges, parteval, tiles, sample, scene, text and
cutpursuit the partition pipeline; _core is their shared plumbing.  Every op requires CUDA(ROCm) tensors and raises otherwise --
there is no CPU fallback in the product path.  This file holds imports only: `ops.NAME` is the public surface."""
from ._core import upload, upload_packed
from .model import (DeviceGraph, EccRnnState, GroupNormState, PointNetState, check_persistent_ecc, colsum, ecc_aggregate_bwd,
                    ecc_aggregate_fwd, eccrnn_backward, eccrnn_forward, gn_backward, gn_forward, gru_cell_bwd, gru_cell_fwd,
                    linear_backward, linear_dgrad, linear_fwd, linear_wgrad, linear_wgrad_bias, lstm_cell_bwd, lstm_cell_fwd,
                    make_eccrnn_cfg, make_gn_cfg, make_pointnet_cfg, persistent_ecc_status, pointnet_backward, pointnet_forward,
                    recover_persistent_ecc)
from .batch import (batch_graph_build, batch_graph_fits, cross_entropy, edge_features, eval_accumulate, gather_rows, load_superpoints,
                    loader_random, set_batch)
from .spgraph import KNN_MAX_K, KnnIndex, compute_geof, knn, prune, sp_graph
from .edges import (EDGE_MAX_D, EdgeGraph, connected_components, contrastive_edge_loss, crosspartition_weights, edge_dist, edge_loss)
from .parteval import (PARTEVAL_MAX_CLASSES, PartitionIndex, boundary_counts, component_label_majority, component_mode,
                       partition_scores, relax_edges, seal_weights)
from .tiles import TILES_MAX_K, TILES_VERTICES_PER_BLOCK, augment_whole, induced_subgraph, neighbourhood_tiles, random_subgraph
from .sample import ResidentSPG, SPGSample, sample_spg
from .scene import (CLASS_COUNT_MAX, PARSED_RECIPES, PLANE_MAX_TRIALS, class_count, parsed_points, plane_elevation, ransac_subsets,
                    scene_stats, scene_structure)
from .text import TEXT_ERRORS, TEXT_MAX_COLS, CloudTextError, CloudTextReader, parse_cloud_text, text_layout
from .cutpursuit import CP_MAX_D, MINCUT_LIMIT, MINCUT_MAX_PULSES, cut_pursuit, min_cut
# the library handle and private names, re-exported for the tests that reach them through `ops` (package code and tools import them from
# _lib and from the owning module)
from .. import _lib
from .._lib import check, lib
from ._core import _ptr, _ptr_array, _req, _stream
from .edges import _edge_forward, _loss_codes
from .parteval import _component_mode, _relax
from .text import _text_roles
from .cutpursuit import _cp_dist, _cp_farthest, _cp_sums
