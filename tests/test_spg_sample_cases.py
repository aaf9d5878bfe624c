"""The supervised loader's sub-sampling without a GPU: on every named case (tests/spg_sample_cases.py) the numpy restatement in
original vertex ids (tests/spg_sample_restatement.py -- the form csrc/spg_sample.hip implements) selects what the host path
selects, and every case has the property it is named for.  Plus the surface of the device path: the CLI flag, ops.sample_spg,
spg.DeviceGraphCache and loader's `device_graphs` parameter."""
import inspect

import numpy as np
import pytest

import spg_sample_cases as C
import spg_sample_restatement as R


def test_the_case_list_is_complete():
    assert sorted(C.cases()) == sorted(C.NAMES)


@pytest.mark.parametrize('name', C.NAMES)
def test_restatement_equals_the_host_path(name):
    case, perm, centres, host = C.cases()[name]
    got = R.sample(case['n'], case['edges'], case['sizes'], perm, centres, case['order'], case['minpts'], case['hardcutoff'])
    for key in ('vids', 'edges', 'kept', 'degs'):
        assert np.array_equal(got[key], host[key]), (name, key)
    assert np.array_equal(case['feats'][got['kept']].view(np.uint32), host['feats'].view(np.uint32))


@pytest.mark.parametrize('name', C.NAMES)
def test_case_has_its_property(name):
    case, perm, centres, host = C.cases()[name]
    assert case['holds'](dict(case=case, perm=perm, centres=centres, host=host)), case['why']


def test_restatement_on_random_graphs():
    """The sweep behind the formulation, at a size that stays quick: random graphs with self-loops and repeated edges over the
    settings' corner values."""
    rs = np.random.RandomState(0)
    for trial in range(60):
        n = int(rs.choice([1, 2, 3, 7, 64, 65, 257]))
        E = int(rs.choice([0, 1, n, 3 * n]))
        case = C._case('random', n, C._random_edges(n, E, trial), int(rs.choice([0, 1, 2, n // 3 + 1, n, 100])), int(rs.choice([0, 1, 3, 50])),
                       int(rs.choice([0, 1, 2, n // 2 + 1, n, n + 5, 512])), seed=trial)
        perm, centres = C.draw(case)
        host = C.host_sample(case)
        got = R.sample(n, case['edges'], case['sizes'], perm, centres, case['order'], case['minpts'], case['hardcutoff'])
        for key in ('vids', 'edges', 'kept', 'degs'):
            assert np.array_equal(got[key], host[key]), (trial, key)


def test_parser_knows_the_flag():
    from superpoint_graph_amd.learning import main
    assert main.build_parser().parse_args([]).spg_sample_device == 0
    assert main.build_parser().parse_args(['--spg_sample_device', '1']).spg_sample_device == 1


def test_device_path_surface_exists():
    from superpoint_graph_amd import ops
    from superpoint_graph_amd.learning import spg
    assert callable(ops.sample_spg) and callable(ops.ResidentSPG)
    assert inspect.isclass(spg.DeviceGraphCache) and inspect.isclass(spg.DeviceSampledGraph)
    assert 'device_graphs' in inspect.signature(spg.loader).parameters
