"""The four EOM-CCSD eigenproblems -- EE, EE left, IP, EA -- live in one slot table on the spin-orbital state (csrc/eom_so.h, DESIGN.md
4.13): what that table must guarantee for all four together, which the other modules check only pairwise (EE beside IP / EA, left beside
right).  On the model o4v6 of np_eom.MODELS (o = 4, v = 6: the smallest on which all four kinds have at least 4 real roots), 2 roots,
max_space = 8:

  * an init of one kind releases that kind's earlier state and no other: the other three step on, their sigma-build counts continuing and
    their omega equal to the bit to those of a second run of the same sequence without the re-init;
  * the re-initialised kind has no guess vectors until it is guessed again, and then serves as a new state;
  * every kind is stale after so_set_amplitudes, and gone -- each with its own message -- after a new so_lambda_init.

No tolerance: everything is equality or a status."""
import numpy as np
import pytest

import np_eom
from afesp_amd.capi import AfespError
from test_gpu_eom import _feed_model

pytestmark = pytest.mark.gpu

NROOTS, MAX_SPACE = 2, 8
STATE = {"ee": "EOM", "left": "left EOM", "ip": "EOM-IP", "ea": "EOM-EA"}     # "no <...> state for the live Lambda state"
KINDS = tuple(STATE)


@pytest.fixture(scope="module")
def eng():
    from afesp_amd.capi import Engine
    e = Engine(0)
    yield e
    e.close()


def _calls(eng, kind):
    """(init, guess, iterate, vector) of a kind"""
    if kind == "ee":
        return eng.so_eom_init, eng.so_eom_guess, eng.so_eom_iterate, eng.so_eom_vector
    if kind == "left":
        return eng.so_eom_left_init, eng.so_eom_left_guess, eng.so_eom_left_iterate, eng.so_eom_left_vector
    sec = eng.EOM_IP if kind == "ip" else eng.EOM_EA
    return (lambda *a: eng.so_eom_ipea_init(sec, *a), lambda: eng.so_eom_ipea_guess(sec), lambda *a: eng.so_eom_ipea_iterate(sec, *a),
            lambda k: eng.so_eom_ipea_vector(sec, k))


def _sequence(eng, c, reinit):
    """Init all four kinds, guess, one step each; then for every kind k in turn: (re-init k, if `reinit`,) one more step of the other
    three, and k from the unit guesses again.  -> {(k, other): (omega, sigma builds of that step)}; every assertion holds in either run."""
    _feed_model(eng, c)
    first, count, steps = {}, {}, {}
    for kind in KINDS:
        init, guess, iterate, _ = _calls(eng, kind)
        init(NROOTS, MAX_SPACE)
        guess()
        omega, _, _, nsigma, _ = iterate(1e-8)
        assert nsigma == NROOTS
        first[kind], count[kind] = omega, nsigma
    for k in KINDS:
        init, guess, iterate, _ = _calls(eng, k)
        if reinit:
            init(NROOTS, MAX_SPACE)
            with pytest.raises(AfespError, match="status 1: .*no guess vectors"):
                iterate(1e-8)
        for other in KINDS:
            if other == k:
                continue
            omega, _, _, nsigma, _ = _calls(eng, other)[2](1e-8)
            assert count[other] < nsigma <= count[other] + NROOTS           # its own count goes on: no more than a correction per root
            steps[k, other] = (omega, nsigma - count[other])
            count[other] = nsigma
        guess()                                                             # k from the unit guesses again: the numbers of its first step
        omega, _, _, nsigma, _ = iterate(1e-8)
        assert np.array_equal(omega, first[k]) and nsigma == NROOTS
        count[k] = nsigma
    return steps


def test_the_four_kinds_are_independent_go_stale_together_and_are_released_together(eng):
    c = np_eom.converged_model("o4v6")
    plain = _sequence(eng, c, reinit=False)
    with_reinit = _sequence(eng, c, reinit=True)
    assert sorted(plain) == sorted(with_reinit) and len(plain) == 12
    for key in plain:
        assert np.array_equal(plain[key][0], with_reinit[key][0]), key      # omega to the bit
        assert plain[key][1] == with_reinit[key][1], key                    # ... from as many sigma builds
    t1, t2 = eng.so_amplitudes()
    eng.so_set_amplitudes(t1, t2)                                           # may have changed t: all four are stale
    for kind in KINDS:
        _, guess, iterate, vector = _calls(eng, kind)
        for call in (lambda: iterate(1e-8), guess, lambda: vector(0)):
            with pytest.raises(AfespError, match="status 21: .*stale"):
                call()
    eng.so_lambda_init(0)                                                   # a new Lambda state: all four are gone, each by its own name
    for kind in KINDS:
        _, guess, iterate, vector = _calls(eng, kind)
        for call in (lambda: iterate(1e-8), guess, lambda: vector(0)):
            with pytest.raises(AfespError, match=f"status 21: .*: no {STATE[kind]} state"):
                call()
