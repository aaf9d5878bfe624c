"""Writes tests/golden/groupnorm_embedder.npz ('layer' and 'third' models) and tests/golden/groupnorm_embedder_group.npz ('group':
one file would pass the repository's size limit for a committed file) from the REFERENCE implementation (needs the reference checkout, located as
tools/gen_edgeloss_golden.py does: SPG_REFERENCE): LocalCloudEmbedder.run_batch of learning/pointnet.py on a stand-alone STNkD
and a PointNet without inner STN, built with norm = 'layer', with norm = 'group' (n_group = 2), and a third, narrow model with
n_group = 2 (with n_group = 4 its 4-wide FC layer has groups of ONE channel: variance exactly 0, rstd = eps^-1/2, and the
reference's own float32 gradients are 6.7e-4 from its float64 ones -- rejected by the assertion below).  The reference file is loaded at run time.  Every parameter is drawn from a seeded generator (randn * 0.3, so the
GroupNorm affines are not 1 / 0 and the STN's projection is not zero).  Each case is run in float32 AND float64; the float64
embeddings and gradients (of every parameter, of the clouds, of the global features; loss = (emb * w).sum(), w a fixed ramp)
are recorded, the gradients rounded once to float32 to keep the file small (2^-24 relative, against a tolerance of 2e-4).  A
case whose float32 reference is not within a quarter of the test tolerances of its float64 result is not a fair yardstick and
aborts the tool.
    python tools/gen_groupnorm_golden.py"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from gen_edgeloss_golden import REF  # noqa: E402

EMB_TOL, GRAD_TOL = 2e-5, 2e-4                      # tests/test_gpu_groupnorm.py
CASES = [(3, 1), (5, 2), (37, 20), (130, 33)]
MODELS = {
    # tag: (STN args, PointNet widths, nfeat, nfeat_global, norm, n_group, cases)
    'layer': ((2, [16, 64], [32, 16]), ([32, 128], [34, 32, 32, 4]), 6, 11, 'layer', 1, CASES),
    'group': ((2, [16, 64], [32, 16]), ([32, 128], [34, 32, 32, 4]), 6, 11, 'group', 2, CASES),
    'third': ((2, [8, 16], [8, 4]), ([16, 32], [16, 8, 4]), 3, 6, 'group', 2, [(9, 7)]),
}


def load_reference():
    spec = importlib.util.spec_from_file_location('ref_pointnet', os.path.join(REF, 'learning', 'pointnet.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def build(P, stn_args, widths, nfeat, nglob, norm, n_group, state=None, gen=None):
    model = torch.nn.Module()
    model.stn = P.STNkD(*stn_args, norm=norm, n_group=n_group)
    model.ptn = P.PointNet(widths[0], widths[1], [], [], nfeat, 0, prelast_do=0, nfeat_global=nglob, is_res=False, norm=norm,
                           n_group=n_group, last_bn=True)
    if state is None:
        state = {k: torch.randn(v.shape, generator=gen) * 0.3 for k, v in model.state_dict().items()}
    model.load_state_dict(state, strict=True)
    return model, state


def make_inputs(rng, n, k, nfeat, nglob_base):
    clouds = rng.uniform(-1, 1, size=(n, nfeat, k)).astype(np.float32)
    if n >= 5:
        clouds[1] = clouds[1, :, :1]                 # a cloud whose points are all equal
    glob = rng.uniform(0, 1, size=(n, nglob_base)).astype(np.float32)
    w = (((np.arange(n * 4).reshape(n, 4) % 7) - 3) / 4.0).astype(np.float32)
    return clouds, glob, w


def run(P, model, clouds, glob, w, dtype):
    model = model.to(dtype).train()
    emb_args = types.SimpleNamespace(ptn_nfeat_stn=2, stn_as_global=1)
    c = torch.from_numpy(clouds).to(dtype).requires_grad_(True)
    g = torch.from_numpy(glob).to(dtype).requires_grad_(True)
    for p in model.parameters():
        p.grad = None
    emb = P.LocalCloudEmbedder(emb_args).run_batch(model, c, g)
    (emb * torch.from_numpy(w).to(dtype)).sum().backward()
    grads = {k: p.grad.detach().double().numpy() for k, p in model.named_parameters()}
    grads['clouds'], grads['clouds_global'] = c.grad.double().numpy(), g.grad.double().numpy()
    return emb.detach().double().numpy(), grads


def grad_error(ours, ref):
    """The max|d| / max|ref| form of tests/test_gpu_local.py::_grad_check."""
    gmax = max(float(np.abs(v).max()) for v in ref.values())
    worst = 0.0
    for k, r in ref.items():
        den = float(np.abs(r).max())
        if den < 1e-5 * gmax:
            assert float(np.abs(ours[k]).max()) <= 1e-5 * gmax, k
            continue
        worst = max(worst, float(np.abs(ours[k] - r).max()) / den)
    return worst


def main():
    if not os.path.isdir(REF):
        sys.exit(f'reference checkout not found at {REF}')
    P = load_reference()
    outs = {'groupnorm_embedder.npz': {}, 'groupnorm_embedder_group.npz': {}}
    for tag, (stn_args, widths, nfeat, nglob, norm, n_group, cases) in MODELS.items():
        out = outs['groupnorm_embedder_group.npz' if tag == 'group' else 'groupnorm_embedder.npz']
        gen = torch.Generator().manual_seed(20 + sorted(MODELS).index(tag))
        model, state = build(P, stn_args, widths, nfeat, nglob, norm, n_group, gen=gen)
        out[f'{tag}/meta'] = np.array([nfeat, nglob, n_group], np.int64)
        out[f'{tag}/norm'] = np.array(norm)
        for k, v in state.items():
            out[f'{tag}/state/{k}'] = v.numpy()
        rng = np.random.default_rng(7 + sorted(MODELS).index(tag))
        for n, k in cases:
            clouds, glob, w = make_inputs(rng, n, k, nfeat, nglob - 4)
            e64, g64 = run(P, build(P, stn_args, widths, nfeat, nglob, norm, n_group, state)[0], clouds, glob, w, torch.float64)
            e32, g32 = run(P, build(P, stn_args, widths, nfeat, nglob, norm, n_group, state)[0], clouds, glob, w, torch.float32)
            ee, ge = float(np.abs(e32 - e64).max()), grad_error(g32, g64)
            finite = np.isfinite(e64).all() and all(np.isfinite(v).all() for v in g64.values())
            print(f'{tag} n={n} k={k}: float32 reference vs float64: emb {ee:.2e} abs, gradients {ge:.2e} rel, finite {bool(finite)}')
            assert finite and ee < EMB_TOL / 4 and ge < GRAD_TOL / 4, 'the reference itself is not a fair yardstick for this case'
            c = f'{tag}/n{n}k{k}'
            out[f'{c}/clouds'], out[f'{c}/clouds_global'], out[f'{c}/w'], out[f'{c}/emb'] = clouds, glob, w, e64
            for name, v in g64.items():
                out[f'{c}/grad/{name}'] = v.astype(np.float32)
    for name, out in outs.items():
        path = os.path.join(ROOT, 'tests', 'golden', name)
        np.savez_compressed(path, **out)
        print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
