"""float64 numpy restatement of the graph contrastive loss of the learned partition (reference supervized_partition/losses.py:
24-64 compute_dist / compute_loss with their gradient, :130-166 compute_weights_XPART in closed form, and connected components
numbered by ascending smallest member).  Pinned to the reference by tests/test_edge_loss_restatement.py through
tests/golden/edge_loss.npz; the GPU tests compare the device kernels with it at sizes the golden does not cover."""
import numpy as np

SMOOTH = 0.999
DELTA = 0.2


def dist(emb, src, tgt, dist_type):
    """losses.py:31-42 in float64 -> (diff [E], d diff / d emb[src] [E, d], d diff / d emb[tgt] [E, d])."""
    a, b = emb[src].astype(np.float64), emb[tgt].astype(np.float64)
    if dist_type == 'euclidian':
        return ((a - b) ** 2).sum(1), 2 * (a - b), -2 * (a - b)
    dot = (a * b).sum(1)
    if dist_type == 'scalar':
        return dot - 1, b, a
    if dist_type == 'intrinsic':
        a0, a1 = np.arccos(SMOOTH), np.arccos(-SMOOTH)
        x = dot * SMOOTH
        diff = (np.arccos(x) - a0) / (a1 - a0) * 3.141592
        dx = -SMOOTH / np.sqrt(1 - x * x) / (a1 - a0) * 3.141592
        return diff, dx[:, None] * b, dx[:, None] * a
    raise ValueError(dist_type)


def loss(diff, is_transition, weights, name, dist_type):
    """losses.py:44-64 in float64 on the given diff -> (loss1, loss2, d (loss1 + loss2) / d diff [E]).  Sub-gradients as
    torch's: clamp(min = 0) passes the gradient where its argument is >= 0."""
    x, w = np.asarray(diff, np.float64), np.asarray(weights, np.float64)
    intra, inter = is_transition == 0, is_transition == 1
    term, dl = np.zeros_like(x), np.zeros_like(x)
    with np.errstate(invalid='ignore', divide='ignore'):
        s = np.sqrt(x + 1e-10)
        if 'tv' in name:
            t, g = w * s, w * 0.5 / s
        elif 'laplacian' in name:
            t, g = w * x, w
        elif 'TVH' in name:
            r = np.sqrt(1 + x / DELTA ** 2)
            t, g = DELTA * w * (r - 1), DELTA * w * 0.5 / r / DELTA ** 2
        else:
            raise ValueError(name)
        term[intra], dl[intra] = t[intra], g[intra]
        if 'zhang' in name:
            beta = 1.0471975512 if dist_type == 'intrinsic' else 1.0
            arg = -w * s + w * beta
            t = np.where(np.isnan(arg), arg, np.maximum(arg, 0))
            g = np.where(np.isnan(arg), arg, np.where(arg >= 0, -w * 0.5 / s, 0.0))
        elif 'TVminus' in name:
            t, g = s * w, w * 0.5 / s
        else:
            raise ValueError(name)
        term[inter], dl[inter] = t[inter], g[inter]
    return term[intra].sum(), term[inter].sum(), dl


def loss_and_grad(emb, src, tgt, is_transition, weights, name, dist_type, scale):
    """diff (float64), loss1, loss2 (from the float32-rounded diff, as the reference's float32 tensor) and the gradient of
    (loss1 + loss2) * scale wrt emb [n, d]."""
    diff, ds, dt = dist(emb, src, tgt, dist_type)
    l1, l2, dl = loss(diff.astype(np.float32), is_transition, weights, name, dist_type)
    g = np.zeros(emb.shape, np.float64)
    np.add.at(g, src, (scale * dl)[:, None] * ds)
    np.add.at(g, tgt, (scale * dl)[:, None] * dt)
    return diff, l1, l2, g


def components(n, src, tgt, active):
    """in_component int64 [n], numbered by ascending smallest member, and the component sizes (min-label propagation with
    pointer jumping; small inputs only)."""
    lab = np.arange(n)
    s, t = np.asarray(src)[np.asarray(active) != 0], np.asarray(tgt)[np.asarray(active) != 0]
    while True:
        m = np.minimum(lab[s], lab[t])
        new = lab.copy()
        np.minimum.at(new, lab[s], m)
        np.minimum.at(new, lab[t], m)
        np.minimum.at(new, s, m)
        np.minimum.at(new, t, m)
        for _ in range(64):
            nxt = new[new]
            if np.array_equal(nxt, new):
                break
            new = nxt
        if np.array_equal(new, lab):
            break
        lab = new
    roots, comp = np.unique(lab, return_inverse=True)
    assert np.array_equal(roots, np.flatnonzero(lab == np.arange(n)))      # the label of a component is its smallest member
    return comp, np.bincount(comp, minlength=len(roots))


def xpart_weights(n, src, tgt, is_transition, pred_in_component, factor):
    """losses.py:130-166 in closed form: float32(1 + min(size_a, size_b) / count(pair) * factor) on transition edges."""
    src, tgt, pred = np.asarray(src), np.asarray(tgt), np.asarray(pred_in_component)
    trans = np.asarray(is_transition) != 0
    comp, size = components(n, src, tgt, (~trans) & (pred[src] == pred[tgt]))
    w = np.ones(len(src), np.float32)
    e = np.flatnonzero(trans)
    a, b = comp[src[e]], comp[tgt[e]]
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    _, inv, cnt = np.unique(lo * len(size) + hi, return_inverse=True, return_counts=True)
    w[e] = (1.0 + np.minimum(size[a], size[b]).astype(np.float64) / cnt[inv].astype(np.float64) * float(factor)).astype(np.float32)
    return w, comp, size
