"""EOM-EE-CCSD excitation energies of a spin-orbital CCSD state: the Davidson driver over Engine.so_eom_* and the labelling of a root
(host code); EOM-IP-CCSD ionisation potentials and EOM-EA-CCSD electron affinities of the same state over
Engine.so_eom_ipea_* (so_eom_ip_solve, so_eom_ea_solve, label_ipea_root); the left eigenvectors of the EE roots, their
biorthonormalisation against the right ones, excited-state and transition densities and oscillator strengths over Engine.so_eom_left_*,
so_eom_ref_coupling and so_eom_density (so_eom_left_solve, biorthonormalise, so_eom_properties, oscillator_strengths); the
left eigenvectors of the IP / EA roots, Dyson orbitals and pole strengths over Engine.so_eom_ipea_left_* and so_eom_ipea_dyson
(so_eom_ip_left_solve, so_eom_ea_left_solve, biorthonormalise_ipea, so_eom_ipea_properties).

The spin-orbital space holds every Ms component: a triplet appears threefold (Ms = 0 and the two spin-flip components Ms = +-1), a singlet
once.  The driver reports the degeneracies and filters nothing."""
from __future__ import annotations

import numpy as np

from .capi import AfespError
from .density import so_spin_order

HARTREE_EV = 27.211386245988
FLAG_CONVERGED, FLAG_COMPLEX = 1, 2


def default_max_space(nroots, nunique):
    """eight vectors per root, at least 2 nroots (what the library asks for)"""
    return max(2 * nroots, min(int(nunique), 8 * nroots))


def _davidson(init, guess, set_guess, iterate, vector, nroots, guesses, tol, maxiter, message):
    """the solve loop of every Davidson state of the library: init() -> max_space, the library's guesses or the caller's, steps until
    every root has converged -> (omega, vectors, info); message names the iteration where maxiter steps do not converge"""
    max_space = init()
    if guesses is None:
        guess()
    else:
        for k, (r1, r2) in enumerate(guesses):
            set_guess(k, r1, r2)
    for it in range(1, maxiter + 1):
        omega, res, flags, nsigma, conv = iterate(tol)
        if conv:
            vectors = [vector(k) for k in range(nroots)]
            info = dict(iterations=it, nsigma=nsigma, resnorm=res, flags=flags, max_space=max_space,
                        r1_norm2=np.array([float(np.sum(x1 * x1)) for x1, _ in vectors]),
                        complex=[k for k in range(nroots) if flags[k] & FLAG_COMPLEX],
                        degeneracy=np.array([int(np.sum(np.abs(omega - w) < 1e-6)) for w in omega]))
            return omega, vectors, info
    raise AfespError(f"the {message} Davidson iteration did not converge in {maxiter} steps (residuals {res})")


def _ee_init(init, eng, nroots, max_space):
    """-> the init() of _davidson for an EE state, right or left: max_space defaults by the unique singles and doubles"""
    def run():
        o, v = eng.so_o, eng.so_v
        ms = max_space if max_space is not None else default_max_space(nroots, o * v + (o * (o - 1) // 2) * (v * (v - 1) // 2))
        init(nroots, ms)
        return ms
    return run


def so_eom_solve(eng, nroots, tol=1e-8, max_space=None, maxiter=100, guesses=None):
    """The nroots lowest EOM-EE-CCSD excitation energies of the engine's spin-orbital state at its current (converged) amplitudes.
    A live Lambda state is needed for its H-bar elements (eng.so_lambda_init, or density.so_lambda_solve); Lambda need not be converged.
    guesses: [(r1, r2)] instead of the unit vectors on the smallest orbital-energy differences.
    -> (omega [nroots], [(x1, x2)] with <x, x> = 1, info) -- info: iterations, nsigma, resnorm, flags, r1_norm2 (sum x1^2 per root: the
    singles weight), complex (roots whose projected value had an imaginary part), degeneracy (roots within 1e-6 Eh of each one).
    Raises AfespError if maxiter steps do not converge."""
    if maxiter < 1:
        raise ValueError("so_eom_solve: maxiter must be at least 1")
    return _davidson(_ee_init(eng.so_eom_init, eng, nroots, max_space), eng.so_eom_guess, eng.so_eom_set_guess, eng.so_eom_iterate,
                     eng.so_eom_vector, nroots, guesses, tol, maxiter, "EOM-CCSD")


def label_root(x1, x2, nbasis, nalpha, nbeta, interleaved):
    """The dominant amplitude of a root and its spin change: -> dict(kind "single" / "double", occ, virt (spatial orbital indices),
    spins_occ, spins_virt (0 alpha, 1 beta), delta_ms, weight).  delta_ms = Ms(excited) - Ms(reference): 0 for spin-conserving
    amplitudes, +-1 for the spin-flip components of a triplet."""
    orb, spin = so_spin_order(nbasis, nalpha, nbeta, interleaved)
    o = nalpha + nbeta
    x1, x2 = np.asarray(x1), np.asarray(x2)
    ms = lambda s: 0.5 - s
    i1 = np.unravel_index(np.argmax(np.abs(x1)), x1.shape)
    i2 = np.unravel_index(np.argmax(np.abs(x2)), x2.shape) if x2.size else None
    if i2 is None or abs(x1[i1]) >= abs(x2[i2]):
        i, a = int(i1[0]), int(i1[1]) + o
        return dict(kind="single", occ=(int(orb[i]),), virt=(int(orb[a]),), spins_occ=(int(spin[i]),), spins_virt=(int(spin[a]),),
                    delta_ms=float(ms(spin[a]) - ms(spin[i])), weight=float(x1[i1] ** 2))
    i, j, a, b = int(i2[0]), int(i2[1]), int(i2[2]) + o, int(i2[3]) + o
    return dict(kind="double", occ=(int(orb[i]), int(orb[j])), virt=(int(orb[a]), int(orb[b])), spins_occ=(int(spin[i]), int(spin[j])),
                spins_virt=(int(spin[a]), int(spin[b])), delta_ms=float(ms(spin[a]) + ms(spin[b]) - ms(spin[i]) - ms(spin[j])),
                weight=float(x2[i2] ** 2))


# ---------------------------------------------------------------------------------------------------------------- left vectors, densities
def dot(x, y):
    """<x, y> = sum x1 y1 + 1/4 sum x2 y2 of two vectors (x1, x2), (y1, y2) on full (i,j,a,b) storage"""
    return float(np.sum(x[0] * y[0]) + 0.25 * np.sum(x[1] * y[1]))


def so_eom_left_solve(eng, right_vectors=None, nroots=None, tol=1e-8, max_space=None, maxiter=100):
    """The left eigenvectors l A = omega l of the nroots lowest EOM-EE-CCSD roots, on a Davidson state of its own beside
    the right-hand one, which is not touched.  right_vectors: the converged right vectors [(r1, r2)] as the left guess (nroots defaults
    to their number) -- the library then follows these states: it returns the Ritz pairs nearest to the roots of the guesses, not the lowest
    ones, so that a lower root the right-hand solve never saw takes no place --; without them the unit vectors of so_eom_solve and the
    lowest roots.  A live Lambda state is needed, as for so_eom_solve.
    -> (omega [nroots], [(l1, l2)] with <l, l> = 1, info) like so_eom_solve.  The vectors are not yet biorthonormal to the right ones:
    see biorthonormalise.  Raises AfespError if maxiter steps do not converge."""
    if maxiter < 1:
        raise ValueError("so_eom_left_solve: maxiter must be at least 1")
    if nroots is None:
        if right_vectors is None:
            raise ValueError("so_eom_left_solve: give nroots or right_vectors")
        nroots = len(right_vectors)
    return _davidson(_ee_init(eng.so_eom_left_init, eng, nroots, max_space), eng.so_eom_left_guess, eng.so_eom_left_set_guess,
                     eng.so_eom_left_iterate, eng.so_eom_left_vector, nroots, None if right_vectors is None else right_vectors[:nroots],
                     tol, maxiter, "left EOM-CCSD")


def clusters(omega, degeneracy_tol=1e-6):
    """index lists of the roots whose omega lie within degeneracy_tol of their neighbour's (omega ascending or not)"""
    order = [int(k) for k in np.argsort(omega, kind="stable")]
    out = []
    for k in order:
        if out and abs(omega[k] - omega[out[-1][-1]]) < degeneracy_tol:
            out[-1].append(k)
        else:
            out.append([k])
    return out


def biorthonormalise(omega, L, R, degeneracy_tol=1e-6):
    """-> new left vectors with <L_j, R_k> = delta_jk inside every cluster of degenerate roots (eigenvectors of different eigenvalues are
    biorthogonal as they are).  Inside a cluster L is replaced by S^-1 L with S_jk = <L_j, R_k>: the three components of a triplet come
    out of the two Davidson iterations in two different bases of their space.  Raises ValueError where a cluster's S is singular
    (condition number above 1e8, with every vector scaled to unit norm): the left and the right solve did not find the same states."""
    if not (len(omega) == len(L) == len(R)):
        raise ValueError("biorthonormalise: omega, L and R differ in length")
    out = [None] * len(L)
    for cl in clusters(np.asarray(omega), degeneracy_tol):
        S = np.array([[dot(L[j], R[k]) for k in cl] for j in cl])
        # (the condition number of the overlaps of the normalised vectors, so that a single root whose two vectors are orthogonal counts)
        nl, nr = [np.sqrt(dot(L[j], L[j])) for j in cl], [np.sqrt(dot(R[k], R[k])) for k in cl]
        sv = np.linalg.svd(S / np.outer(nl, nr), compute_uv=False) if min(nl + nr) > 0.0 else np.zeros(1)
        if not sv[-1] * 1e8 >= max(1.0, sv[0]):
            raise ValueError(f"biorthonormalise: the overlap of the left and right vectors of the roots {cl} is singular "
                             f"(singular values {sv}): the two solves found different states")
        Si = np.linalg.inv(S)
        for a, j in enumerate(cl):                                           # S^-1 L: (S^-1 S)_jk = delta_jk
            out[j] = (sum(Si[a, b] * L[m][0] for b, m in enumerate(cl)), sum(Si[a, b] * L[m][1] for b, m in enumerate(cl)))
    return out


def so_eom_properties(eng, omega, L, R, lam):
    """Per root k, from biorthonormal left vectors L (biorthonormalise), right vectors R and the converged ground-state lam = (l1, l2):
    -> [dict(r0, density, g0k, gk0)].  r0 = <0| H-bar R_k |0> / omega_k; density is the correlation part of the excited state's
    one-particle density (afesp_amd.density.spatial_blocks adds the reference), g0k = <0| (1 + Lambda) [p+ q] R_k |0> and gk0 =
    <0| L_k [p+ q] |0> the two transition densities, all symmetrised, (o+v) x (o+v) in the state's spin-orbital order."""
    c = eng.so_eom_ref_coupling(np.stack([r[0] for r in R]), np.stack([r[1] for r in R]))
    out = []
    for k, w in enumerate(omega):
        r0 = float(c[k] / w)
        out.append(dict(r0=r0, density=eng.so_eom_density(0.0, L[k], r0, R[k]), g0k=eng.so_eom_density(1.0, lam, r0, R[k]),
                        gk0=eng.so_eom_density(0.0, L[k], 1.0, None)))
    return out


def oscillator_strengths(omega, g0k, gk0, dipole_so):
    """f_k = 2/3 omega_k sum_x (mu^x . gamma^0k)(mu^x . gamma^k0).  dipole_so: the three Cartesian components of the dipole operator as
    symmetric matrices over the state's spin orbitals, in its order (afesp_amd.density.so_spin_order).  The program reads no dipole
    integrals: the operator is the caller's, in the same molecular orbitals as the state."""
    dipole_so = [np.asarray(m, dtype=np.float64) for m in dipole_so]
    if len(dipole_so) != 3 or any(m.shape != np.shape(g0k[0]) or not np.allclose(m, m.T, rtol=0.0, atol=1e-12 * max(1.0, np.max(np.abs(m))))
                                  for m in dipole_so):
        raise ValueError("oscillator_strengths: dipole_so is three symmetric matrices of the densities' shape")
    return np.array([2.0 / 3.0 * w * sum(float(np.sum(m * a)) * float(np.sum(m * b)) for m in dipole_so) for w, a, b in zip(omega, g0k, gk0)])


def left_table(omega_left, omega_right, info):
    """The lines the Fortran host prints for eom_left: root, omega_left in Eh and eV, |omega_left - omega_right|, residual, sigma builds"""
    lines = ["  root   omega(left) / Eh   omega(left) / eV   |left-right|     residual"]
    for k, w in enumerate(omega_left):
        lines.append(f"  {k + 1:4d}  {w:16.10f}  {w * HARTREE_EV:16.8f}  {abs(w - omega_right[k]):11.3e}  {info['resnorm'][k]:11.3e}")
    lines.append(f"  left sigma builds: {info['nsigma']}")
    return "\n".join(lines)


# ---------------------------------------------------------------------------------------------------------------- triples correction
INTRUDER_GAP = 0.05    # Eh.  A diagnostic constant, not a tolerance: a state whose omega comes this close to a triples denominator is flagged


def triples_min_gap(omega, levels, o):
    """|omega - (e_a + e_b + e_c - e_i - e_j - e_k)| per root at the smallest such difference, that of the three highest occupied and the
    three lowest virtual levels: the denominator an excitation energy from below meets first"""
    lev = np.asarray(levels, dtype=np.float64)
    eo, ev = np.sort(lev[:o]), np.sort(lev[o:])
    omega = np.atleast_1d(np.asarray(omega, dtype=np.float64))
    if eo.size < 3 or ev.size < 3:
        return np.full(omega.size, np.inf)
    return np.abs(omega - float(ev[:3].sum() - eo[-3:].sum()))


def so_eom_triples_correction(eng, omega, L, R, t_begin=0, t_end=None, levels=None):
    """The non-iterative triples correction to the EOM-EE-CCSD excitation energies omega from biorthonormal left vectors L
    (biorthonormalise) and right vectors R, all states in one library call -> (delta, omega + delta, info).  Refuses vectors with
    |<L_k, R_k> - 1| > 1e-8.  info["min_gap"]: the smallest |omega_k - (e_a + e_b + e_c - e_i - e_j - e_k)| from the levels (the state's
    Fock diagonal, fetched unless given); info["intruder"]: the roots whose gap is below INTRUDER_GAP.  A sub-range [t_begin, t_end) of
    the triples gives that shard's part of delta (ranks add theirs up)."""
    omega = np.atleast_1d(np.asarray(omega, dtype=np.float64))
    if not (len(omega) == len(L) == len(R)):
        raise ValueError("so_eom_triples_correction: omega, L and R differ in length")
    for k in range(len(omega)):
        ov = dot(L[k], R[k])
        if abs(ov - 1.0) > 1e-8:
            raise ValueError(f"so_eom_triples_correction: <L, R> of root {k + 1} is {ov:.12f}, not 1: biorthonormalise the vectors first")
    delta = eng.so_eom_t(omega, L, R, t_begin, t_end)
    if levels is None:
        levels = eng.so_levels()
    gap = triples_min_gap(omega, levels, eng.so_o)
    info = dict(min_gap=gap, intruder=[k for k in range(len(omega)) if gap[k] < INTRUDER_GAP])
    return delta, omega + delta, info


def triples_table(omega, delta, info):
    """The lines the Fortran host prints for eom_triples: root, omega, delta, omega + delta in Eh and eV, one line per flagged state"""
    lines = ["  root        omega / Eh   delta omega / Eh   omega+delta / Eh   omega+delta / eV"]
    for k, w in enumerate(omega):
        lines.append(f"  {k + 1:4d}  {w:16.10f}  {delta[k]:16.10f}  {w + delta[k]:16.10f}  {(w + delta[k]) * HARTREE_EV:16.8f}")
    for k in info["intruder"]:
        lines.append(f"  root {k + 1}: omega is within {info['min_gap'][k]:.4f} Eh of a triples denominator (below {INTRUDER_GAP} Eh): "
                     "the correction is not reliable")
    return "\n".join(lines)


# ---------------------------------------------------------------------------------------------------------------- EOM-IP / EOM-EA
SECTOR_IP, SECTOR_EA = 1, 2


def ipea_nunique(sector, o, v):
    """i, then (i < j, a) / a, then (i, a < b)"""
    return o + (o * (o - 1) // 2) * v if sector == SECTOR_IP else v + o * (v * (v - 1) // 2)


def _so_eom_ipea_solve(eng, sector, nroots, tol, max_space, maxiter, guesses):
    if maxiter < 1:
        raise ValueError("so_eom_ip_solve / so_eom_ea_solve: maxiter must be at least 1")
    def init():
        ms = max_space if max_space is not None else default_max_space(nroots, ipea_nunique(sector, eng.so_o, eng.so_v))
        eng.so_eom_ipea_init(sector, nroots, ms)
        return ms
    return _davidson(init, lambda: eng.so_eom_ipea_guess(sector), lambda k, r1, r2: eng.so_eom_ipea_set_guess(sector, k, r1, r2),
                     lambda t: eng.so_eom_ipea_iterate(sector, t), lambda k: eng.so_eom_ipea_vector(sector, k), nroots, guesses, tol, maxiter,
                     "EOM-CCSD")


def so_eom_ip_solve(eng, nroots, tol=1e-8, max_space=None, maxiter=100, guesses=None):
    """The nroots lowest EOM-IP-CCSD ionisation potentials omega = E(N-1) - E(N) of the engine's spin-orbital state, as so_eom_solve finds
    excitation energies: a live Lambda state is needed.  Vectors are (x1 (o,), x2 (o,o,v)) with sum x1^2 + 1/2 sum x2^2 = 1; r1_norm2 is the
    one-hole weight.  The library's guesses carry a small admixture of every unique amplitude, so that a root in another Ms block or irreducible
    representation than the smallest diagonal elements is found too.  Nothing is filtered: a closed-shell reference shows every doublet twofold (info["degeneracy"])."""
    return _so_eom_ipea_solve(eng, SECTOR_IP, nroots, tol, max_space, maxiter, guesses)


def so_eom_ea_solve(eng, nroots, tol=1e-8, max_space=None, maxiter=100, guesses=None):
    """The nroots lowest EOM-EA-CCSD electron affinities omega = E(N+1) - E(N); vectors are (x1 (v,), x2 (o,v,v)).  See so_eom_ip_solve."""
    return _so_eom_ipea_solve(eng, SECTOR_EA, nroots, tol, max_space, maxiter, guesses)


def label_ipea_root(sector, x1, x2, nbasis, nalpha, nbeta, interleaved):
    """The dominant amplitude of an IP or EA root: -> dict(kind "1h" / "2h1p" or "1p" / "2p1h", occ, virt (spatial orbital indices),
    spins_occ, spins_virt (0 alpha, 1 beta), delta_ms, weight).  delta_ms = Ms(target) - Ms(reference): -+1/2 for the removal or the
    attachment of an alpha / beta electron where the other amplitudes conserve spin."""
    orb, spin = so_spin_order(nbasis, nalpha, nbeta, interleaved)
    o = nalpha + nbeta
    x1, x2 = np.asarray(x1), np.asarray(x2)
    ms = lambda s: 0.5 - s
    i1 = int(np.argmax(np.abs(x1)))
    i2 = np.unravel_index(np.argmax(np.abs(x2)), x2.shape) if x2.size else None
    if i2 is None or abs(x1[i1]) >= abs(x2[i2]):
        occ, virt = ((i1,), ()) if sector == SECTOR_IP else ((), (i1 + o,))
        kind, weight = ("1h" if sector == SECTOR_IP else "1p"), float(x1[i1] ** 2)
    else:
        occ, virt = ((int(i2[0]), int(i2[1])), (int(i2[2]) + o,)) if sector == SECTOR_IP else ((int(i2[0]),), (int(i2[1]) + o, int(i2[2]) + o))
        kind, weight = ("2h1p" if sector == SECTOR_IP else "2p1h"), float(x2[i2] ** 2)
    return dict(kind=kind, occ=tuple(int(orb[p]) for p in occ), virt=tuple(int(orb[p]) for p in virt),
                spins_occ=tuple(int(spin[p]) for p in occ), spins_virt=tuple(int(spin[p]) for p in virt),
                delta_ms=float(sum(ms(spin[p]) for p in virt) - sum(ms(spin[p]) for p in occ)), weight=weight)


# ---------------------------------------------------------------------------------------------------------------- IP / EA: left vectors, Dyson orbitals
def dot_ipea(x, y):
    """<x, y> = sum x1 y1 + 1/2 sum x2 y2 of two vectors of a sector on full storage"""
    return float(np.sum(x[0] * y[0]) + 0.5 * np.sum(x[1] * y[1]))


def _so_eom_ipea_left_solve(eng, sector, right_vectors, nroots, tol, max_space, maxiter):
    if maxiter < 1:
        raise ValueError("so_eom_ip_left_solve / so_eom_ea_left_solve: maxiter must be at least 1")
    if nroots is None:
        if right_vectors is None:
            raise ValueError("so_eom_ip_left_solve / so_eom_ea_left_solve: give nroots or right_vectors")
        nroots = len(right_vectors)
    def init():
        ms = max_space if max_space is not None else default_max_space(nroots, ipea_nunique(sector, eng.so_o, eng.so_v))
        eng.so_eom_ipea_left_init(sector, nroots, ms)
        return ms
    return _davidson(init, lambda: eng.so_eom_ipea_left_guess(sector), lambda k, l1, l2: eng.so_eom_ipea_left_set_guess(sector, k, l1, l2),
                     lambda t: eng.so_eom_ipea_left_iterate(sector, t), lambda k: eng.so_eom_ipea_left_vector(sector, k), nroots,
                     None if right_vectors is None else right_vectors[:nroots], tol, maxiter, "left EOM-CCSD")


def so_eom_ip_left_solve(eng, right_vectors=None, nroots=None, tol=1e-8, max_space=None, maxiter=100):
    """The left eigenvectors l A = omega l of EOM-IP-CCSD roots, on a Davidson state of its own beside the sector's
    right-hand one, which is not touched.  right_vectors: the converged right vectors [(r1, r2)] as the left guess (nroots defaults to
    their number) -- the library then follows the states of the guesses, as so_eom_left_solve; without them the library's guesses and the
    lowest roots.  -> (omega, [(l1, l2)] with <l, l> = 1, info) like so_eom_ip_solve; not yet biorthonormal: biorthonormalise_ipea."""
    return _so_eom_ipea_left_solve(eng, SECTOR_IP, right_vectors, nroots, tol, max_space, maxiter)


def so_eom_ea_left_solve(eng, right_vectors=None, nroots=None, tol=1e-8, max_space=None, maxiter=100):
    """The left eigenvectors of EOM-EA-CCSD roots.  See so_eom_ip_left_solve."""
    return _so_eom_ipea_left_solve(eng, SECTOR_EA, right_vectors, nroots, tol, max_space, maxiter)


def biorthonormalise_ipea(omega, L, R, degeneracy_tol=1e-6):
    """biorthonormalise with the sectors' metric <x, y> = sum x1 y1 + 1/2 sum x2 y2: -> new left vectors with <L_j, R_k> = delta_jk inside
    every cluster of degenerate roots.  Every doublet of a closed-shell reference is a twofold cluster whose two Davidson iterations end
    in two different bases, so S^-1 L with S_jk = <L_j, R_k> is the normal path here.  Raises ValueError where a cluster's S is singular
    (condition number above 1e8 with every vector scaled to unit norm): the left and the right solve did not find the same states.
    Roots of a cluster whose right vectors are equal to the bit are one state: the library gives both members of a pair of roots that
    rounding split into omega +- i epsilon the pair's one real vector (flag FLAG_COMPLEX).  S is formed over the distinct states, with the
    left vector of each state's first root, and the other roots of the state receive the same left vector -- a vector of the doublet's
    space like any other, whose pole strength is the doublet's."""
    if not (len(omega) == len(L) == len(R)):
        raise ValueError("biorthonormalise_ipea: omega, L and R differ in length")
    out = [None] * len(L)
    for members in clusters(np.asarray(omega), degeneracy_tol):
        cl, first = [], {}
        for j in members:
            same = [k for k in cl if np.array_equal(R[j][0], R[k][0]) and np.array_equal(R[j][1], R[k][1])]
            first[j] = same[0] if same else j
            if not same:
                cl.append(j)
        S = np.array([[dot_ipea(L[j], R[k]) for k in cl] for j in cl])
        nl, nr = [np.sqrt(dot_ipea(L[j], L[j])) for j in cl], [np.sqrt(dot_ipea(R[k], R[k])) for k in cl]
        sv = np.linalg.svd(S / np.outer(nl, nr), compute_uv=False) if min(nl + nr) > 0.0 else np.zeros(1)
        if not sv[-1] * 1e8 >= max(1.0, sv[0]):
            raise ValueError(f"biorthonormalise_ipea: the overlap of the left and right vectors of the roots {cl} is singular "
                             f"(singular values {sv}): the two solves found different states")
        Si = np.linalg.inv(S)
        for a, j in enumerate(cl):
            out[j] = (sum(Si[a, b] * L[m][0] for b, m in enumerate(cl)), sum(Si[a, b] * L[m][1] for b, m in enumerate(cl)))
        for j in members:
            out[j] = out[first[j]]
    return out


def so_eom_ipea_properties(eng, sector, L, R):
    """Per root k, from biorthonormal left vectors L (biorthonormalise_ipea) and right vectors R of the sector, all roots in one library
    call: -> [dict(dyson_left, dyson_right, pole_strength)].  The Dyson vectors run over the o + v spin orbitals in the state's order,
    dyson_left[p] = <0| L_k e^-T a_p e^T |0>, dyson_right[p] = <0| (1 + Lambda) e^-T a_p^+ e^T R_k |0> for IP (a_p^+ / a_p for EA), with the
    converged lambda of the engine's live Lambda state; pole_strength = sum_p dyson_left[p] dyson_right[p].  Inside a degenerate cluster
    only the sum of the pole strengths is independent of the basis the cluster's vectors came out in."""
    if len(L) != len(R):
        raise ValueError("so_eom_ipea_properties: L and R differ in length")
    gl, gr = eng.so_eom_ipea_dyson(sector, (np.stack([x[0] for x in L]), np.stack([x[1] for x in L])),
                                   (np.stack([x[0] for x in R]), np.stack([x[1] for x in R])))
    return [dict(dyson_left=gl[k], dyson_right=gr[k], pole_strength=float(np.dot(gl[k], gr[k]))) for k in range(len(L))]


def dyson_spin_parts(gamma, nbasis, nalpha, nbeta, interleaved):
    """A Dyson vector over the state's spin orbitals (afesp_amd.density.so_spin_order) -> (alpha, beta) parts over the nbasis spatial
    orbitals: an ionisation or attachment of definite Ms has one of them zero"""
    orb, spin = so_spin_order(nbasis, nalpha, nbeta, interleaved)
    gamma = np.asarray(gamma, dtype=np.float64)
    if gamma.shape != (len(orb),):
        raise ValueError(f"dyson_spin_parts: the vector has shape {gamma.shape}, the state {len(orb)} spin orbitals")
    parts = np.zeros((2, nbasis))
    parts[spin, orb] = gamma
    return parts[0], parts[1]


def ipea_left_table(omega_left, omega_right, info, pole):
    """The lines the Fortran host prints for eom_ipea_left: root, omega_left in Eh and eV, |omega_left - omega_right|, residual, pole
    strength, and the sigma builds"""
    lines = ["  root   omega(left) / Eh   omega(left) / eV   |left-right|     residual   pole strength"]
    for k, w in enumerate(omega_left):
        lines.append(f"  {k + 1:4d}  {w:16.10f}  {w * HARTREE_EV:16.8f}  {abs(w - omega_right[k]):11.3e}  {info['resnorm'][k]:11.3e}  {pole[k]:14.10f}")
    lines.append(f"  left sigma builds: {info['nsigma']}")
    return "\n".join(lines)


def table(omega, info):
    """The lines the Fortran host prints: root, omega in Eh and eV, |r1|^2, residual, sigma builds"""
    lines = ["  root        omega / Eh        omega / eV     |r1|^2     residual"]
    for k, w in enumerate(omega):
        lines.append(f"  {k + 1:4d}  {w:16.10f}  {w * HARTREE_EV:16.8f}  {info['r1_norm2'][k]:9.6f}  {info['resnorm'][k]:11.3e}")
    lines.append(f"  sigma builds: {info['nsigma']}")
    return "\n".join(lines)


# ---------------------------------------------------------------------------------------------------------------- triples correction, IP / EA
def ipea_triples_min_gap(sector, omega, levels, o):
    """|omega - D_eps| per root at the smallest D_eps of the sector's 3h2p / 3p2h determinants: e_a + e_b - e_i - e_j - e_k from the three
    highest occupied and the two lowest virtual levels (IP), e_a + e_b + e_c - e_i - e_j from the two highest occupied and the three lowest
    virtual ones (EA) -- the denominator a root from below meets first"""
    lev = np.asarray(levels, dtype=np.float64)
    eo, ev = np.sort(lev[:o]), np.sort(lev[o:])
    omega = np.atleast_1d(np.asarray(omega, dtype=np.float64))
    no, nv = (3, 2) if sector == SECTOR_IP else (2, 3)
    if eo.size < no or ev.size < nv:
        return np.full(omega.size, np.inf)
    return np.abs(omega - float(ev[:nv].sum() - eo[-no:].sum()))


def _so_eom_ipea_triples_correction(eng, sector, omega, L, R, begin, end, levels):
    who = "so_eom_ip_triples_correction" if sector == SECTOR_IP else "so_eom_ea_triples_correction"
    omega = np.atleast_1d(np.asarray(omega, dtype=np.float64))
    if not (len(omega) == len(L) == len(R)):
        raise ValueError(f"{who}: omega, L and R differ in length")
    for k in range(len(omega)):
        ov = dot_ipea(L[k], R[k])
        if abs(ov - 1.0) > 1e-8:
            raise ValueError(f"{who}: <L, R> of root {k + 1} is {ov:.12f}, not 1: biorthonormalise_ipea the vectors first")
    delta = eng.so_eom_ipea_t(sector, omega, L, R, begin, end)
    if levels is None:
        levels = eng.so_abs_levels()      # (2 - 3 or 3 - 2 levels: a common shift does not cancel)
    gap = ipea_triples_min_gap(sector, omega, levels, eng.so_o)
    info = dict(min_gap=gap, intruder=[k for k in range(len(omega)) if gap[k] < INTRUDER_GAP])
    return delta, omega + delta, info


def so_eom_ip_triples_correction(eng, omega, L, R, begin=0, end=None, levels=None):
    """The non-iterative 3h2p correction to the EOM-IP-CCSD ionisation potentials omega from biorthonormal left vectors L
    (biorthonormalise_ipea) and right vectors R, all roots in one library call -> (delta, omega + delta, info).  Refuses vectors with
    |<L_k, R_k> - 1| > 1e-8 in the sector's metric.  info["min_gap"]: the smallest |omega_k - (e_a + e_b - e_i - e_j - e_k)| from the
    levels (the state's Fock diagonal, fetched unless given); info["intruder"]: the roots whose gap is below INTRUDER_GAP.  A sub-range
    [begin, end) of the triples i<j<k gives that shard's part of delta (ranks add theirs up).  triples_table prints the result."""
    return _so_eom_ipea_triples_correction(eng, SECTOR_IP, omega, L, R, begin, end, levels)


def so_eom_ea_triples_correction(eng, omega, L, R, begin=0, end=None, levels=None):
    """The same for the EOM-EA-CCSD electron affinities: the 3p2h correction, the gap |omega_k - (e_a + e_b + e_c - e_i - e_j)|, shards over
    the pairs i<j"""
    return _so_eom_ipea_triples_correction(eng, SECTOR_EA, omega, L, R, begin, end, levels)
