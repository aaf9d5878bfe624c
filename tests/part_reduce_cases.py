"""The cases whose BITS tests/golden/part_reduce_parent.npz pins (tools/gen_part_reduce_golden.py writes it, on the commit before the
partition units' reductions moved into csrc/spg_part.h; tests/test_gpu_part_reduce_bits.py compares): every op of the partition
pipeline that goes through the fixed-order reduction of DESIGN.md section 4.11e, at the sizes at which that shape changes -- a
partial wave, one wave, a partial workgroup, several workgroups, the 1024th workgroup (n = 262 144) and the first grid-stride
element (262 145).  Inputs are regenerated from np.random.RandomState; none is stored.  Small results are recorded whole,
per-point arrays as SHA-256 digests (uint8 [32]).

CASES: name -> function(ops) -> {field: numpy array}."""
import hashlib

import numpy as np
import torch

SCENE_SIZES = (1, 63, 64, 65, 255, 256, 257, 1025, 262144, 262145)
PARSED_SIZES = KNN_SIZES = (257, 262145)
PLANE_SIZES = (1025, 4097, 262145)
EDGE_SIZES = (1, 255, 257, 65537)
NAN_SIZES = (65, 262145)          # the NaN sits at index n - 1: the last lane of a partial wave, the grid-stride round
ROOM = np.array([10.0, 8.0, 3.0], np.float32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def digest(t):
    a = np.ascontiguousarray(host(t) if torch.is_tensor(t) else t)
    return np.frombuffer(hashlib.sha256(a.tobytes()).digest(), np.uint8).copy()


def room(n, offset=0.0, seed=0):
    """n points uniform in the 10 x 8 x 3 room, float32; offset 1e3 moves them to where the float64 sums of float32 values round"""
    rs = np.random.RandomState(1000 + seed + n % 100003)
    return (rs.rand(n, 3).astype(np.float32) * ROOM + np.float32(offset)).astype(np.float32)


def floor_room(n):
    """a room whose low points (less than 0.5 above the lowest) number at least 1025: all of them at n = 1025, 60 % beyond"""
    rs = np.random.RandomState(2000 + n % 100003)
    xyz = rs.rand(n, 3).astype(np.float32) * ROOM
    n_floor = n if n <= 1025 else (6 * n) // 10
    tilt = 0.01 * xyz[:n_floor, 0] - 0.005 * xyz[:n_floor, 1]
    xyz[:n_floor, 2] = (0.1 + tilt + 0.02 * rs.randn(n_floor)).astype(np.float32)
    return xyz[rs.permutation(n)].copy()


def knn_table(ops, xyz_d):
    """ops.knn with k = 4; below five points as many neighbours as there are, and at n = 1 the one-column table [[0]]"""
    n = int(xyz_d.shape[0])
    if n == 1:
        return torch.zeros(1, 1, dtype=torch.int32, device='cuda')
    return ops.knn(xyz_d, min(4, n - 1), distances=False)[0]


def scene_case(n, offset):
    def run(ops):
        xyz = dev(room(n, offset))
        s32, s64, centroid = ops.scene_stats(xyz, with_distance=True)
        ids = dev(np.random.RandomState(n % 100003).randint(0, 5, n).astype(np.int64))
        st = ops.scene_structure(xyz, knn_table(ops, xyz), 1, ids=ids, id_mode='given')
        return {'stats_f32': host(s32), 'stats_f64': host(s64), 'centroid': host(centroid),
                'elevation': digest(st['elevation']), 'xyn': digest(st['xyn'])}
    return run


def parsed_case(n):
    def run(ops):
        rs = np.random.RandomState(3000 + n % 100003)
        xyz = dev(room(n, 0.0, seed=1))
        rgb = dev(rs.randint(0, 256, (n, 3)).astype(np.uint8))
        geof = dev(rs.rand(n, 4).astype(np.float32))
        cuts = np.sort(rs.randint(0, n + 1, 6))
        comp_off = np.concatenate([[0], cuts, [n]]).astype(np.int64)
        comp_idx = dev(rs.permutation(n).astype(np.int64))
        points, centroid, off = ops.parsed_points('s3dis', xyz, rgb, comp_off, comp_idx, geof=geof)
        return {'points': digest(points), 'centroid': host(centroid), 'offsets': np.asarray(off, np.int64)}
    return run


def plane_case(n):
    def run(ops):
        p = ops.plane_elevation(dev(floor_room(n)))            # subsets: ransac_subsets(n_low, 100, 0)
        assert p['n_low'] >= 1025, p['n_low']
        return {'coef': host(p['coef']), 'intercept': host(p['intercept']), 'threshold': host(p['threshold']),
                'counts': np.array([p['n_low'], p['n_trials'], p['best_trial']], np.int64),
                'elevation': digest(p['elevation']), 'inlier_mask': digest(p['inlier_mask'])}
    return run


def edge_case(E):
    def run(ops):
        rs = np.random.RandomState(4000 + E % 100003)
        n = max(2, E // 4)
        graph = ops.EdgeGraph(dev(rs.randint(0, n, E).astype(np.int64)), dev(rs.randint(0, n, E).astype(np.int64)), n)
        emb = dev(rs.randn(n, 8).astype(np.float32)).requires_grad_(True)
        trans = dev((rs.rand(E) < 0.4).astype(np.uint8))
        weights = dev(rs.rand(E).astype(np.float32))
        l1, l2, diff = ops.contrastive_edge_loss(emb, graph, trans, weights)
        (l1 + 2.0 * l2).backward()
        return {'loss': np.array([l1.item(), l2.item()], np.float32), 'diff': digest(diff), 'grad': digest(emb.grad)}
    return run


def knn_case(n):
    def run(ops):
        rs = np.random.RandomState(5000 + n % 100003)
        xyz = dev(room(n, 0.0, seed=2))
        idx, dist = ops.knn(xyz, 4)
        rgb = dev(rs.randint(0, 256, (n, 3)).astype(np.uint8))
        labels = dev(rs.randint(0, 6, n).astype(np.uint8))
        objects = dev(rs.randint(0, 8, n).astype(np.int32))
        pruned = ops.prune(xyz, 0.1, rgb=rgb, labels=labels, objects=objects, n_labels=5, n_objects=7)
        out = {'knn_idx': digest(idx), 'knn_dist': digest(dist), 'prune_voxels': np.array([pruned[0].shape[0]], np.int64)}
        out.update({f'prune_{name}': digest(t) for name, t in zip(('xyz', 'rgb', 'labels', 'objects'), pruned)})
        return out
    return run


CASES = {}
for _n in SCENE_SIZES:
    CASES[f'scene_{_n}'] = scene_case(_n, 0.0)
    CASES[f'scene_{_n}_offset'] = scene_case(_n, 1e3)
CASES.update({f'parsed_{n}': parsed_case(n) for n in PARSED_SIZES})
CASES.update({f'plane_{n}': plane_case(n) for n in PLANE_SIZES})
CASES.update({f'edgeloss_{E}': edge_case(E) for E in EDGE_SIZES})
CASES.update({f'knn_prune_{n}': knn_case(n) for n in KNN_SIZES})
