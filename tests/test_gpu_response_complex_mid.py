"""The fused pass of the complex linear mode (davidson_cfused_kernel) at a mid-size vector: (o, v) = (10, 46), built as
tests/test_gpu_response_mid.py builds its shapes, nvec = o v + o^2 v^2 = 212060 -- every one of the 128 blocks of partials makes several
trips and the last trip is ragged -- without a dense Jacobian.  One operator at z = 0.1 + 0.05 i and -z, a few steps, no convergence asked:
the residual norm the step reports is held against the residual rebuilt from the fetched P and Q with Engine.so_eom_sigma,

    rho_re = xi + A P - omega P + gamma Q,      rho_im = A Q - omega Q - gamma P,      |rho|^2 = <rho_re, rho_re> + <rho_im, rho_im>,

within 1e-10 max(1, |xi|)."""
import numpy as np
import pytest

import np_eom
from test_gpu_lambda import _build_case, _feed
from test_response_cpu import random_symmetric

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from afesp_amd.capi import Engine
    e = Engine(0)
    yield e
    e.close()


def test_reported_residual_is_the_residual_of_the_fetched_vectors(eng):
    c = _build_case("rhf_10_46", "rhf", 28, 5, 5, 204)
    o, v = c["o"], c["v"]
    assert (o, v) == (10, 46)
    _feed(eng, c)
    eng.so_lambda_init(0)
    X = random_symmetric(np.random.default_rng(204), o + v)
    xi = eng.so_response_xi(X)
    z = 0.1 + 0.05j
    eng.so_response_init_complex(X[None], [z, -z], 16)
    for it in range(3):
        res, nsigma, conv = eng.so_response_iterate(1e-12)
    assert 6 <= nsigma <= 4 * 3 and not conv                                # Re and Im of both systems every step, less what was dropped
    bound = 1e-10 * max(1.0, float(np.sqrt(np_eom.dot(*xi, *xi))))
    for g, zz in enumerate((z, -z)):
        R = eng.so_response_vector_complex(0, g)
        P, Q = (R[0].real.copy(), R[1].real.copy()), (R[0].imag.copy(), R[1].imag.copy())
        sP, sQ = eng.so_eom_sigma(*P), eng.so_eom_sigma(*Q)
        rre = [xi[k] + sP[k] - zz.real * P[k] + zz.imag * Q[k] for k in range(2)]
        rim = [sQ[k] - zz.real * Q[k] - zz.imag * P[k] for k in range(2)]
        rebuilt = float(np.sqrt(np_eom.dot(*rre, *rre) + np_eom.dot(*rim, *rim)))
        print("z", zz, "reported", res[g, 0], "rebuilt", rebuilt, "difference", abs(res[g, 0] - rebuilt), "bound", bound)
        assert abs(res[g, 0] - rebuilt) <= bound
        assert np.array_equal(R[1], -R[1].transpose(1, 0, 2, 3)) and np.array_equal(R[1], -R[1].transpose(0, 1, 3, 2))
        assert np.any(Q[1]) and rebuilt > 0.0
