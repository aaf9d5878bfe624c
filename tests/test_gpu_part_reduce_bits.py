"""GPU: the fixed-order reductions of the partition units (csrc/spg_part.h) give the bits that the commit
before they were stated once gave.  tests/golden/part_reduce_parent.npz (tools/gen_part_reduce_golden.py, run on that commit) holds
them; the inputs are regenerated from np.random.RandomState (tests/part_reduce_cases.py).  Equality is of bytes: float results are
compared through their bit patterns, per-point arrays through SHA-256.  And a NaN in the last element, which only the last lane
of a partial wave (n = 65) or the grid-stride round (n = 262 145) reads, is reported by every unit that checks."""
import os

import numpy as np
import pytest
import torch

import part_reduce_cases as C
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def parent():
    with np.load(os.path.join(GOLDEN, 'part_reduce_parent.npz')) as z:
        return {k: z[k] for k in z.files}


def test_the_record_names_its_commit_and_covers_every_case(parent):
    assert len(str(parent['parent_commit'])) == 40
    assert {k.split('/')[0] for k in parent if '/' in k} == set(C.CASES)


@pytest.mark.parametrize('name', list(C.CASES))
def test_bits_equal_the_parent_commit(hip, parent, name):
    from superpoint_graph_amd import ops
    got = C.CASES[name](ops)
    assert set(got) == {k.split('/')[1] for k in parent if k.startswith(name + '/')}
    for field, value in got.items():
        want = parent[f'{name}/{field}']
        assert value.dtype == want.dtype and value.shape == want.shape, (name, field)
        assert value.tobytes() == want.tobytes(), (name, field, value, want)


@pytest.mark.parametrize('n', C.NAN_SIZES)
def test_nan_in_the_last_element_is_reported(hip, n):
    from superpoint_graph_amd import ops
    bad = C.room(n)
    bad[n - 1, 1] = np.nan
    bad = C.dev(bad)
    message = 'Input contains NaN or infinity.'
    with pytest.raises(ValueError, match=message):
        ops.scene_stats(bad, with_distance=True)
    with pytest.raises(ValueError, match=message):
        ops.scene_structure(bad, torch.zeros(n, 1, dtype=torch.int32, device='cuda'), 1,
                            ids=torch.zeros(n, dtype=torch.int64, device='cuda'), id_mode='given')
    with pytest.raises(ValueError, match=message):
        ops.plane_elevation(bad)
    with pytest.raises(ValueError, match='knn: the input contains NaN or infinity'):
        ops.KnnIndex(bad).self_query(4)
