"""The arm step kernels against the recorded bits of the parent of the change that made the table's
normal a compile-time constant in their contact rows (tests/golden/make_table_normal_bits.py names
the commit, the four cases and how each drive was chosen): a robot point's normal, g1rb and g1w are
neither stored nor read back there, plane_space is not evaluated, and the rows' Jacobian entries
are Jv.z, -Jv.y and Jv.x instead of three-term dot products -- with the signed zeros those gave, so
observation, q, qd and the contact cache (feature ids and normal impulses) are the same words at
every recorded step.  No tolerance.

Coverage is asserted from the recorded file, so the comparison cannot pass because nothing
happened: one wave (4 consecutive envs) holds an env with exactly 2 robot points, one with exactly
1 and one with none; some env holds both end spheres of a two-sphere capsule; a point is recorded at
the plane's height beside the table (on_table false); and in the limit case an env touches while
its elbow sits at its upper limit."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location(
    "make_table_normal_bits",
    os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_table_normal_bits.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)


@pytest.fixture(scope="module")
def pg():
    import panda_gym_amd as pg

    pg.load_native()
    return pg


@pytest.fixture(scope="module")
def golden():
    with np.load(G.GOLDEN) as z:
        return {k: z[k] for k in z.files}


def test_golden_covers_point_counts_ends_plane_and_limit(golden):
    assert len(golden) == sum(len(G.NAMES) * len(G.RECORD[c]) for c in G.CASES)
    cov = G.coverage(golden)
    print(cov)
    assert all(cov.values()), cov


@pytest.mark.parametrize("case", G.CASES)
def test_bits_equal_the_parents(pg, golden, case):
    got = G.run(pg, case)
    want = {k: v for k, v in golden.items() if k.startswith(case + "/")}
    assert sorted(got) == sorted(want) and len(want) == len(G.NAMES) * len(G.RECORD[case])
    bad = []
    for k in sorted(want):
        assert got[k].dtype == np.uint32 and got[k].shape == want[k].shape, k
        diff = int(np.count_nonzero(got[k] != want[k]))
        print(k, "words differing:", diff, "of", want[k].size)
        if diff:
            bad.append((k, diff))
    assert not bad, bad
