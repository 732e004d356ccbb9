"""The step kernels against the recorded bits of the parent of the row-per-lane Cholesky change
(tests/golden/make_parent_bits.py names the commit): the dynamics' and the IK's 7x7 factorisation
and forward substitution run one row per lane with chol7 / chol7_solve's products in their order,
so observation, q and qd are the same bits after 5, 10, 20 and 30 pressing-down steps, in both
control modes' kernels.  The run crosses from no contact to two table points per env."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location(
    "make_parent_bits", os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_parent_bits.py"))
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


@pytest.mark.parametrize("env_id", G.ENV_IDS)
def test_bits_equal_the_parents(pg, golden, env_id):
    got = G.run(pg, env_id)
    want = {k: v for k, v in golden.items() if k.startswith(env_id + "/")}
    assert sorted(got) == sorted(want) and len(want) == 3 * len(G.RECORD)
    bad = []
    for k in sorted(want):
        assert got[k].dtype == np.uint32 and got[k].shape == want[k].shape, k
        diff = int(np.count_nonzero(got[k] != want[k]))
        print(k, "words differing:", diff, "of", want[k].size)
        if diff:
            bad.append((k, diff))
    assert not bad, bad
