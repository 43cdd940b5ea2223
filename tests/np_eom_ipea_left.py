"""Reference for the left-hand side of EOM-IP-CCSD and EOM-EA-CCSD on the spin-orbital CCSD state (no GPU): the left sigma build of
either sector, and the Dyson orbitals of a left and a right vector.  Layouts, metric and sectors are np_eom_ipea's.

Left sigma.  sigma_L(l) = A^T l with the transpose in the sector's metric: <l, sigma(r)> = <sigma_L(l), r>.  Two forms:

  * lsigma_definition: the ghost embedding of np_eom_ipea into np_eom_left.lsigma_definition (A^T of the enlarged EE problem on the packed
    embedded vector), read from the ghost components, with no hand-derived term;
  * lsigma_explicit: np_eom_ipea's sigma transposed term by term over the H-bar elements of np_lambda.hbar -- the form the device code
    follows, with the same intermediates and the same letters.

Dyson orbitals.  In the system enlarged by the ghost g, with l' / r' / lambda' / t' the embedded vectors and D the symmetrised matrix of
np_eom_left (density_definition), for a pair <l, r> = 1

    gamma_L[p] = 2 D[g,p] at the argument pair (0, l'; 1, 0)        <0| L e^-T a_p e^T |0>           (IP; a_p^+ for EA)
    gamma_R[p] = 2 D[g,p] at the argument pair (1, lambda'; 0, r')  <0| (1 + Lambda) e^-T a_p^+ e^T R |0>  (IP; a_p for EA)

over all o + v spin orbitals p, occupied first (only one of the orientations g -> p / p -> g is non-zero: hence the 2).  The pole strength
is sum_p gamma_L[p] gamma_R[p].  Two forms:

  * dyson_definition: central differences of np_eom_left.F in the Fock elements f_gp = f_pg of the enlarged system;
  * dyson_explicit: the restriction of np_eom_left.density_explicit to those components, as the device builds it.
"""
from __future__ import annotations

import numpy as np

import np_eom_ipea as X
import np_eom_left
import np_lambda
import np_rocc
from np_ucc import E

IP, EA = X.IP, X.EA


# ---------------------------------------------------------------------------------------------------------------- embedding
def embed(sector, o, v, x1, x2):
    """the vector of the enlarged EE problem: IP g = virtual v, x'1[i,g] = x_i, x'2[i,j,a,g] = -x'2[i,j,g,a] = x_ija; EA g = occupied o,
    x'1[g,a] = x_a, x'2[i,g,a,b] = -x'2[g,i,a,b] = x_iab"""
    if sector == IP:
        R1, R2 = np.zeros((o, v + 1)), np.zeros((o, o, v + 1, v + 1))
        R1[:, v] = x1
        R2[:, :, :v, v] = x2
        R2[:, :, v, :v] = -x2
    else:
        R1, R2 = np.zeros((o + 1, v)), np.zeros((o + 1, o + 1, v, v))
        R1[o] = x1
        R2[:o, o] = x2
        R2[o, :o] = -x2
    return R1, R2


def embed_plain(sector, o, v, t1, t2):
    """t or lambda in the enlarged system: zero on every component with g"""
    if sector == IP:
        T1, T2 = np.zeros((o, v + 1), t1.dtype), np.zeros((o, o, v + 1, v + 1), t2.dtype)
        T1[:, :v], T2[:, :, :v, :v] = t1, t2
    else:
        T1, T2 = np.zeros((o + 1, v), t1.dtype), np.zeros((o + 1, o + 1, v, v), t2.dtype)
        T1[:o], T2[:o, :o] = t1, t2
    return T1, T2


def restrict(sector, o, v, S1, S2):
    """-> (x1, x2, leak: the largest |component without g, or with g twice|)"""
    if sector == IP:
        leak = max(np.max(np.abs(S1[:, :v])), np.max(np.abs(S2[:, :, :v, :v])), np.max(np.abs(S2[:, :, v, v])))
        return S1[:, v].copy(), S2[:, :, :v, v].copy(), float(leak)
    leak = max(np.max(np.abs(S1[:o])), np.max(np.abs(S2[:o, :o])), np.max(np.abs(S2[o, o])))
    return S1[o].copy(), S2[:o, o].copy(), float(leak)


def enlarged(sector, g, f, o):
    """-> (g', f', o') with the ghost spin orbital"""
    n = f.shape[0]
    gg, fg = X._ghost(g, f, o, n if sector == IP else o)
    return gg, fg, (o if sector == IP else o + 1)


# ---------------------------------------------------------------------------------------------------------------- left sigma
def lsigma_definition(sector, g, f, o, t1, t2, l1, l2):
    """-> (sigma_L1, sigma_L2, leak).  A^T of the enlarged problem couples the ghost components of l to ghost components only, as A does"""
    v = f.shape[0] - o
    gg, fg, og = enlarged(sector, g, f, o)
    cc = np_rocc.ROCC(gg, fg, og)
    T1, T2 = embed_plain(sector, o, v, t1, t2)
    S1, S2 = np_eom_left.lsigma_definition(cc, T1, T2, *embed(sector, o, v, l1, l2))
    return restrict(sector, o, v, S1, S2)


def lsigma_matrix(sector, cc, t1, t2, l1, l2, A=None):
    """np_eom_ipea.matrix^T on the packed vector (packed, the metric is the plain dot product)"""
    A = A if A is not None else X.matrix(sector, cc, t1, t2)
    return X.unpack(sector, A.T @ X.pack(sector, l1, l2), cc.o, cc.v)


def ip_lsigma_explicit(cc, t1, t2, l1, l2, I=None):
    I = I if I is not None else np_lambda.hbar(cc, t1, t2)
    eo, ev = X.levels(cc)
    Hov, Hoo, Hvv = I["Hov"], I["Hoo"], I["Hvv"]
    s1 = -E("mi,i->m", Hoo, l1) + 0.5 * E("maij,ija->m", I["Hovoo"], l2) - eo * l1
    G = 0.5 * E("ija,ijae->e", l2, t2)
    W = (0.5 * E("mnij,ije->mne", I["Hoooo"], l2) + E("mna,ae->mne", l2, Hvv) + E("mnie,i->mne", I["Hooov"], l1)
         + E("a,mnae->mne", G, cc.oovv))
    A = E("mja,naej->mne", l2, I["Hovvo"]) - E("mje,nj->mne", l2, Hoo) - E("m,ne->mne", l1, Hov)
    d = eo[:, None, None] + eo[None, :, None] - ev[None, None, :]
    return s1, W + A - A.transpose(1, 0, 2) - d * l2


def ea_lsigma_explicit(cc, t1, t2, l1, l2, I=None):
    I = I if I is not None else np_lambda.hbar(cc, t1, t2)
    eo, ev = X.levels(cc)
    Hov, Hoo, Hvv = I["Hov"], I["Hoo"], I["Hvv"]
    s1 = E("ae,a->e", Hvv, l1) - 0.5 * E("ieab,iab->e", I["Hvvvo"], l2) + ev * l1
    G = 0.5 * E("iab,imab->m", l2, t2)
    Xt = E("iab,mb->iam", l2, t1)
    Q = E("iab,mnab->imn", l2, I["tau"])
    W = (0.5 * E("iab,abef->ief", l2, cc.vvvv) + 0.25 * E("imn,mnef->ief", Q, cc.oovv) + E("m,mief->ief", G, cc.oovv)
         - E("im,mef->ief", Hoo, l2) - E("aief,a->ief", I["Hvovv"], l1) - E("iam,amef->ief", Xt, cc.vovv))
    B = E("mab,ibem->iae", l2, I["Hovvo"]) + E("iab,be->iae", l2, Hvv) - E("a,ie->iae", l1, Hov)
    d = eo[:, None, None] - ev[None, :, None] - ev[None, None, :]
    return s1, W + B - B.transpose(0, 2, 1) - d * l2


def lsigma_explicit(sector, cc, t1, t2, l1, l2, I=None):
    return (ip_lsigma_explicit if sector == IP else ea_lsigma_explicit)(cc, t1, t2, l1, l2, I)


# ---------------------------------------------------------------------------------------------------------------- Dyson orbitals
def _ghost_row(sector, g, f, o, T, l0, l, r0, r, eps=2.0 ** -6):
    """2 D[g,p] of np_eom_left's symmetrised matrix over p = the o + v spin orbitals of the system itself, occupied first"""
    n = f.shape[0]
    gg, fg, og = enlarged(sector, g, f, o)
    at = n if sector == IP else o
    out = np.zeros(n)
    for p in range(n):
        q = p if (sector == IP or p < o) else p + 1      # (EA: g sits between the occupied and the virtual orbitals)
        x = np.zeros((n + 1, n + 1))
        x[at, q] = x[q, at] = eps
        fp = np_eom_left.F(np_rocc.ROCC(gg, fg + x, og), *T, l0, l, r0, r)
        fm = np_eom_left.F(np_rocc.ROCC(gg, fg - x, og), *T, l0, l, r0, r)
        out[p] = (fp - fm) / (2.0 * eps)                 # = 2 . 1/2 (dF/df_gp + dF/df_pg)
    return out


def dyson_definition(sector, g, f, o, t1, t2, lam1, lam2, l=None, r=None):
    """-> (gamma_L or None, gamma_R or None) of the sector vectors l = (l1, l2), r = (r1, r2)"""
    v = f.shape[0] - o
    T = embed_plain(sector, o, v, t1, t2)
    gl = gr = None
    if l is not None:
        gl = _ghost_row(sector, g, f, o, T, 0.0, embed(sector, o, v, *l), 1.0, None)
    if r is not None:
        gr = _ghost_row(sector, g, f, o, T, 1.0, embed_plain(sector, o, v, lam1, lam2), 0.0, embed(sector, o, v, *r))
    return gl, gr


def dyson_explicit(sector, cc, t1, t2, lam1, lam2, l=None, r=None):
    """IP   gamma_L[i] = l_i                      gamma_L[a] = l_i t_ia - 1/2 l_mnf t_mnaf
            gamma_R[a] = u_a = lam_ia r_i - 1/2 lam_mnaf r_mnf
            gamma_R[m] = r_m + lam_ia r_ima - t_ma u_a - Goo_mj r_j,       Goo_mj = 1/2 t_mnef lam_jnef
       EA   gamma_L[a] = l_a                      gamma_L[m] = -l_a t_ma + 1/2 l_nef t_mnef
            gamma_R[i] = u_i = -lam_ia r_a + 1/2 lam_inef r_nef
            gamma_R[e] = r_e + lam_ia r_iae + u_j t_je - r_b Gvv_be,       Gvv_be = 1/2 t_mnef lam_mnbf"""
    gl = gr = None
    if sector == IP:
        if l is not None:
            l1, l2 = l
            gl = np.concatenate([l1, E("i,ia->a", l1, t1) - 0.5 * E("mnf,mnaf->a", l2, t2)])
        if r is not None:
            r1, r2 = r
            u = E("ia,i->a", lam1, r1) - 0.5 * E("mnaf,mnf->a", lam2, r2)
            Goo = 0.5 * E("mnef,jnef->mj", t2, lam2)
            gr = np.concatenate([r1 + E("ia,ima->m", lam1, r2) - E("ma,a->m", t1, u) - E("mj,j->m", Goo, r1), u])
    else:
        if l is not None:
            l1, l2 = l
            gl = np.concatenate([-E("a,ma->m", l1, t1) + 0.5 * E("nef,mnef->m", l2, t2), l1])
        if r is not None:
            r1, r2 = r
            u = -E("ia,a->i", lam1, r1) + 0.5 * E("inef,nef->i", lam2, r2)
            Gvv = 0.5 * E("mnef,mnbf->be", t2, lam2)
            gr = np.concatenate([u, r1 + E("ia,iae->e", lam1, r2) + E("j,je->e", u, t1) - E("b,be->e", r1, Gvv)])
    return gl, gr


def pole_strength(gl, gr):
    return float(np.dot(gl, gr))


# ---------------------------------------------------------------------------------------------------------------- exact models
def eigen_pairs(sector, cc, t1, t2, I=None):
    """every root of the sector's matrix over the unique amplitudes with its right vector and the biorthonormal left one (the rows of the
    inverse of the eigenvector matrix: <L_j, R_k> = delta_jk also inside a degenerate cluster) -> (omega ascending, L, R) on full storage"""
    A = X.matrix(sector, cc, t1, t2, I)
    w, V = np.linalg.eig(A)
    order = np.argsort(w.real, kind="stable")
    w, V = w[order].real, V[:, order].real
    Vi = np.linalg.inv(V)
    o, v = cc.o, cc.v
    return w, [X.unpack(sector, Vi[k], o, v) for k in range(len(w))], [X.unpack(sector, V[:, k], o, v) for k in range(len(w))]


def cluster_sums(omega, values, tol=1e-6):
    """[(mean omega, sum of values, size)] over the clusters of roots within tol of their neighbour, omega ascending"""
    out = []
    for k in np.argsort(omega, kind="stable"):
        if out and abs(omega[k] - out[-1][0][-1]) < tol:
            out[-1][0].append(omega[k])
            out[-1][1].append(values[k])
        else:
            out.append(([omega[k]], [values[k]]))
    return [(float(np.mean(w)), float(np.sum(p)), len(w)) for w, p in out]


def fci_ip_two_electrons(h, chem):
    """Ionising the two-electron ground state c (over |p alpha, q beta>) into the one-electron state u_k of h with either spin:
    -> (omega_k = eps_k - E0 ascending, strength per twofold cluster: |c^T u_k|^2 + |c u_k|^2); the strengths sum to 2"""
    w, c = np_eom_left.fci_two_electron_states(h, chem)
    eps, U = np.linalg.eigh(h)
    return eps - w[0], np.array([np.sum((c[0].T @ U[:, k]) ** 2) + np.sum((c[0] @ U[:, k]) ** 2) for k in range(len(eps))])


def one_electron_reference(h, chem):
    """One alpha electron in the lowest eigenvector of h, everything in the eigenbasis of h: the reference is exact (t = 0, E1 = eps_0)
    -> (eps, chem', fa, fb)"""
    eps, U = np.linalg.eigh(h)
    chem_e = np.einsum("pqrs,pa,qb,rc,sd->abcd", chem, U, U, U, U, optimize=True)
    fa, fb = np_rocc.fock_ro(np.diag(eps), chem_e, 1, 0)
    return eps, chem_e, fa, fb


def fci_ea_one_electron(eps, chem_e):
    """Attaching an electron to that reference: the Ms = 0 two-electron states c_k over |p alpha, q beta> of the same Hamiltonian
    -> (E_k - eps_0 ascending, sum_q c_k[0,q]^2, singlet?) -- a triplet's Ms = +-1 components lie at the same energy, so only a singlet's
    root is non-degenerate in the EA sector"""
    w, c = np_eom_left.fci_two_electron_states(np.diag(eps), chem_e)
    return w - eps[0], np.array([np.sum(ck[0] ** 2) for ck in c]), [np_eom_left.fci_is_singlet(ck) for ck in c]
