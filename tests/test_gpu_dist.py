"""GPU: the data-parallel mode with TWO ranks (both on the one GPU of the test box, gloo rendezvous on 127.0.0.1).
With synchronised BatchNorm the 2-rank step must reproduce the reference's single-process step on the 2-scene batch
(golden fixture); with per-rank statistics it must not (different normalisation)."""
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _run_world2(sync, native=False, mode='slots', fused=0):
    port = _free_port()
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE='2', MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port),
                   HSA_ENABLE_IPC_MODE_LEGACY='0', SPG_NATIVE_RCCL='1' if native else '0')
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, '_sync_bn_worker.py'), str(sync), mode, str(fused)], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = []
    for p in procs:
        try:
            out, _ = p.communicate(timeout=240)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        outs.append(out)
    for p, out in zip(procs, outs):
        assert p.returncode == 0, out[-3000:]
    return outs


@pytest.mark.parametrize('mode,fused', [('slots', 0), ('slots', 1), ('finalize', 0)])
def test_two_ranks_sync_bn_reproduce_single_process_reference(hip, mode, fused):
    """mode 'slots' (round 5): the ranks all-reduce the exact fixed-point statistics slots between producer and consumer launch --
    statistics folds, fused convolution backward, one-pass first layers stay on, and (fused = 1) the whole step is ONE library call
    (spg_train_step); mode 'finalize': the fp64 sums of a finalize launch per layer (rounds 1-4)."""
    outs = _run_world2(1, mode=mode, fused=fused)
    assert all(f'sync=1 mode={mode} fused={fused}' in o for o in outs)


def test_two_ranks_local_bn_is_a_different_model(hip):
    _run_world2(0)


def test_two_gpus_native_rccl_sync_bn_reproduce_single_process_reference(hip):
    """Two ranks on two GPUs, every collective of the step (26 BatchNorm all-reduces + the flat gradient all-reduce) issued
    by libspg_hip's own RCCL communicator: must reproduce the reference's single-process 2-scene step.  Needs a
    multi-GPU node (skipped on the 1-GPU test box; RCCL refuses two ranks on one device)."""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip('needs >= 2 GPUs')
    outs = _run_world2(1, native=True)
    assert all('sync=1' in o for o in outs)


def test_native_rccl_single_rank(hip):
    """The library's own RCCL communicator at world size 1 (the 1-GPU box): bootstrap, the fp32 arena all-reduce and the
    synchronised-BatchNorm all-reduces issued from C -- the training step must be bit-identical to the local one."""
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', MASTER_PORT=str(_free_port()), HSA_ENABLE_IPC_MODE_LEGACY='0')
    out = subprocess.run([sys.executable, os.path.join(HERE, '_native_rccl_worker.py')], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and 'native rccl ok' in out.stdout, (out.stdout + out.stderr)[-3000:]


def test_rccl_collectives_single_rank_smoke(hip):
    """every collective of the data-parallel mode on the RCCL backend (one rank: the test box has one GPU)"""
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', MASTER_PORT=str(_free_port()), HSA_ENABLE_IPC_MODE_LEGACY='0')
    out = subprocess.run([sys.executable, os.path.join(os.path.dirname(HERE), 'tools', 'rccl_smoke.py')], env=env,
                         capture_output=True, text=True, timeout=240)
    assert out.returncode == 0 and 'rccl smoke ok' in out.stdout, (out.stdout + out.stderr)[-3000:]


@pytest.mark.parametrize('mode', ['finalize', 'slots'])
def test_sync_bn_world1_equals_local_bn_at_full_size(hip, mode):
    """At world size 1 the synchronised modes must reproduce the local step bit for bit.  'finalize' (reduce -> callback -> finish,
    here on top of the sliced reduction of the large layers): same fp64 sums, same finishing arithmetic as the local finalize
    path; 'slots' (round 5: the statistics slots themselves are all-reduced, the row counts come from a device buffer): the plain
    per-rank step with every fast path on."""
    import types

    import torch
    import torch.nn.functional as F

    sys.path.insert(0, os.path.dirname(HERE))
    import bench
    from superpoint_graph_amd import dist as spd
    from superpoint_graph_amd.learning import pointnet
    dev = torch.device('cuda')
    model = bench.build_model('gru_10_0,f_13', dev).train()
    state0 = {k: v.detach().clone() for k, v in model.state_dict().items()}
    targets, GIs, flag, clouds, diam, _ = bench.make_batch([0], 1000, 5000)
    clouds_d, diam_d, label = clouds.to(dev), diam.to(dev), targets[:, 0].to(dev)
    model.ecc.set_info(GIs, 1)

    def run():
        model.load_state_dict(state0)
        model.zero_grad()
        emb_er = pointnet.CloudEmbedder(types.SimpleNamespace(cuda=1, ptn_mem_monger=1))
        emb = emb_er.run(model, None, flag, clouds_d, diam_d)
        out = model.ecc(emb)
        F.cross_entropy(out, label).backward()
        emb_er.bw_hook()
        return out.detach().clone(), {k: p.grad.detach().clone() for k, p in model.named_parameters()}, \
            {k: v.detach().clone() for k, v in model.state_dict().items() if 'running' in k}

    # (the local run with the separate data-gradient / weight-gradient launches the synchronised mode uses: the fused backward of
    #  the 64 / 128-input-channel layers -- spg_tune key 14, tests/test_gpu_bwdpair.py -- sums dW in another order)
    # ... and the first two convolutions / the first convolution's backward as the separate launches (keys 17, 18: round 5's one-pass
    # kernels take the first layer's statistics from the Gram matrix -- not bit-identical to sums over rounded outputs)
    keys = (14, 17, 18) if mode == 'finalize' else ()
    old = [hip.spg_tune(k, 1) for k in keys]
    try:
        out0, g0, r0 = run()
    finally:
        for k, v in zip(keys, old):
            hip.spg_tune(k, v)
    st = spd.enable_sync_bn(dev, mode=mode)
    try:
        out1, g1, r1 = run()
    finally:
        spd.disable_sync_bn()
    assert st['error'] is None and st['calls'] >= 26
    assert torch.equal(out0, out1)
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k
    for k in r0:
        assert torch.equal(r0[k], r1[k]), k


def test_bench_two_ranks_with_roofline_pass(hip):
    """bench.py launched the way the driver launches it for N > 1 (torch.distributed.run, one process per rank); both ranks
    share the test box's single GPU and talk over gloo, which exercises every rank-dependent branch (sharding, barriers,
    the collectives of the step and of the instrumented pass, rank-0 reporting)."""
    import json
    root = os.path.dirname(HERE)
    port = _free_port()
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
           '--master-port', str(port), os.path.join(root, 'bench.py'), '--gpus', '2', '--steps', '3', '--warmup', '2', '--full',
           '--backend', 'gloo', '--device-index', '0', '--n-sp', '200', '--n-edges', '800']
    out = subprocess.run(cmd, env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0'), capture_output=True, text=True, timeout=400)
    assert out.returncode == 0, (out.stdout + out.stderr)[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, out.stdout[-2000:]                        # exactly one JSON line, from rank 0
    d = json.loads(lines[0])
    assert d['n_gpus'] == 2 and d['value'] > 0 and d['config']['superpoints_per_step'] == 400
    assert 'roofline' in d and 'skipped' in d['cpu_baseline'] and 'value' not in d['cpu_baseline']      # (N > 1: marked, not silently absent)


@pytest.mark.parametrize('launcher', ['torchrun', 'self'])
@pytest.mark.parametrize('sync_bn', [0, 1])
def test_bench_two_ranks_control_flow(hip, sync_bn, launcher):
    """bench.py for N > 1 on the one GPU of the test box with the gloo backend: the data-parallel control flow (scene sharding,
    barrier + max-over-ranks timing, weighted gradient all-reduce, rank 0 prints ONE JSON line with the whole-job value)
    without needing two devices.  launcher = torchrun: as torch.distributed.run starts it (one process per rank);
    launcher = self: the PLAIN command `python bench.py --gpus 2 ...` with no WORLD_SIZE in the environment -- the script has
    to start its own ranks (that command used to print an N = 1 line)."""
    import json
    root = os.path.dirname(HERE)
    tail = [os.path.join(root, 'bench.py'), '--gpus', '2', '--steps', '4', '--warmup', '2', '--full',
            '--backend', 'gloo', '--device-index', '0', '--sync-bn', str(sync_bn), '--no-cpu-baseline', '--no-forward-only', '--no-roofline']
    if launcher == 'torchrun':
        cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
               '--master-port', str(_free_port())] + tail
    else:
        cmd = [sys.executable] + tail
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT')}
    out = subprocess.run(cmd, env=dict(env, HSA_ENABLE_IPC_MODE_LEGACY='0'), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    assert d['n_gpus'] == 2 and d['ranks_seen'] == 2 and d['steps'] == 4 and d['scaling'] == 'weak' and d['unit'] == 'superpoints/s'
    assert d['config']['superpoints_per_step'] == 2000 and d['value'] > 0
    assert abs(d['value'] - 2000 / (d['ms_per_step'] * 1e-3)) < 1e-6 * d['value']
    assert ('synchronised' in d['config']['batchnorm']) == bool(sync_bn) and d['batchnorm'] == ('sync' if sync_bn else 'per-rank')
    assert d['allreduce_us_per_step'] > 0
    assert d['self_check']['persistent_errors'] == 0 and d['self_check']['grads_finite']
    assert len(d['config']['workload']) < 120 and d['config']['workload'].startswith('gru_10_0,f_13')


def test_bench_refuses_more_ranks_than_gpus(hip):
    """`python bench.py --gpus N` on a node with fewer than N GPUs must fail loudly instead of printing a smaller job's line."""
    import torch
    n = torch.cuda.device_count() + 1
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK')}
    out = subprocess.run([sys.executable, os.path.join(os.path.dirname(HERE), 'bench.py'), '--gpus', str(n), '--steps', '2', '--warmup', '1'],
                         env=env, capture_output=True, text=True, timeout=200)
    assert out.returncode != 0 and 'refusing' in out.stderr and not [ln for ln in out.stdout.splitlines() if ln.startswith('{')]
