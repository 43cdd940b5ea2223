// integrals.h -- the integral layer: everything between "AO integrals arrive" and "packed MO integrals are resident" (integrals.hip).
#pragma once
#include "ccsd.h"

namespace afesp {

struct Solver;   // solver.h: told when a packed array its spin-free state may read goes away

inline int64_t npair_of(int64_t n) { return n * (n + 1) / 2; }
inline int64_t neri_of(int64_t n) { return npair_of(npair_of(n)); }

// Which form a transform of basis size n takes, and the leading dimension of the squared-up temporaries that goes with it (the
// half-unpacked AO integrals a Fock build leaves for it included) -- decided ONCE per call, from one snapshot of the knob table: the
// transforms on the LDS-DMA GEMM keep columns of 16 ceil(n / 16) doubles -- every column then starts on a 128-byte line, for the GEMM's
// K steps and for the layout kernels' runs alike (n = 220: 39.2 -> 36 ms per transform; n = 224 ran FASTER than n = 220 before,
// profiles/r06_ao2mo_alignment_scan.txt) -- every other form keeps n.
struct Ao2moForm {
    bool blocked;   // slab by slab (AFESP_AO2MO_BLOCKED=0 / 1; default: where the n^2 npair temporaries pass 2^31 doubles)
    bool use_tg;    // the LDS-DMA GEMM: even n, and from n = 96 on (its tile has 128 rows: below that most of a tile is padding and the
                    // transform is launch-bound anyway); AFESP_AO2MO_TG=0 / 1: never / for every even n >= 16 (tests, A/B runs)
    bool pair;      // up to 64 basis functions: the LDS-resident pair transform (AFESP_AO2MO_PAIR=0: the gather-GEMM form)
    int64_t ld;
    // open_shell: afesp_ao2mo_ump2's forms -- no LDS-DMA one, dense columns, the pair transform up to n = 64 whatever the knobs say
    explicit Ao2moForm(int64_t n, bool open_shell = false);
};

// The integrals resident in a context.  The member functions are the only code that writes these fields.
struct Integrals {
    double* ao = nullptr;   // packed AO integrals (afesp_read_eri_text / afesp_set_eri / afesp_synthetic_ao)
    int64_t ao_n = 0;       // nbasis they belong to
    double* mo = nullptr;   // packed MO integrals left by afesp_ao2mo_mp2 / afesp_mo_window
    int64_t mo_n = 0;
    // the UHF MO integrals left by afesp_ao2mo_ump2 for afesp_ccsd_uso_init: alpha-alpha and beta-beta packed, alpha-beta full
    // (kept apart from mo: the RHF calls never see them, nor they the RHF ones)
    double *uhf_aa = nullptr, *uhf_bb = nullptr, *uhf_ab = nullptr;
    int64_t uhf_n = 0;
    // scratch "ao2mo_a" holds the half-unpacked AO integrals (ij|KL) of this basis size / leading dimension / scratch epoch
    int64_t half_n = 0, half_ld = 0, half_epoch = -1;
    // the LDS-DMA transforms' temporaries whose padding rows are known to be zero: buffers, extents, scratch epoch
    const double *pad_a = nullptr, *pad_b = nullptr;
    int64_t pad_n = 0, pad_ld = 0, pad_epoch = -1;

    // doubles of a squared-up temporary, the same for a Fock build and the transform after it, which so finds the build's very buffer (16 of
    // slack: the LDS-DMA GEMM reads whole 16-element K steps, i.e. up to Kc - n elements past a column's end -- the next column's, finite,
    // times the zero padding of C -- and past the tensor's end behind the last one)
    static int64_t temp_size(int64_t n, int64_t ld) { return ld * n * npair_of(n) + 16; }

    double* adopt_ao(Context& cx, int64_t n);   // a fresh device array to fill; the old one is released, the half-unpacked copy stale
    void upload_ao(Context& cx, int64_t n, const double* host);
    bool half_valid(const Context& cx, int64_t n, int64_t ld) const { return half_n == n && half_ld == ld && half_epoch == cx.scratch_epoch; }
    // (ij|KL) in scratch "ao2mo_a", columns of `ld` doubles as the transform will want them: built by the first Fock build of an SCF
    const double* half_unpacked(Context& cx, int64_t n, int64_t& ld);
    void half_restamp(const Context& cx) { half_epoch = cx.scratch_epoch; }   // (growing a Fock work buffer moves the epoch, not u)
    void half_overwritten() { half_n = 0; }
    void padding_overwritten() { pad_n = 0; }   // (a form that writes the temporaries densely: zeroed padding rows are data now)
    void zero_padding(Context& cx, double* a, double* b, int64_t n, int64_t ld);
    void release_uhf(Context& cx);
    void adopt_uhf(Context& cx, int64_t n);            // the three blocks for basis size n (kept where they are of that size)
    void swap_uhf(Context& cx, double* aa, double* bb, double* ab, int64_t n);   // three filled blocks take the resident ones' place (afesp_read_fcidump_uhf)
    void window_uhf(Context& cx, int64_t n_act, int64_t lo);   // the orbitals [lo, lo + n_act) of the three blocks, as afesp_mo_window's of mo
    void drop_mo(Context& cx, Solver& sv);            // back to the arena; a solver state initialised from them can no longer form <ef|ab>
    double* replace_mo(Context& cx, Solver& sv, int64_t n);   // the array a transform writes: the resident one if it has the size
    void set_mo(double* packed, int64_t n) { mo = packed; mo_n = n; }
};

// the bodies of the entry points of the same names (capi.hip checks the arguments); each returns the energy / the count it reports
// build_fock (src/hf.f90:349-385) and the unrestricted pair on the resident packed AO integrals of basis size n; host matrices n x n
void build_fock(Context& cx, Integrals& in, int64_t n, const double* density, const double* hcore, double* fock);
void build_fock_uhf(Context& cx, Integrals& in, int64_t n, const double* dens_a, const double* dens_b, const double* hcore, double* fock_a,
                    double* fock_b);
double ao2mo_mp2(Context& cx, Integrals& in, Solver& sv, int64_t n, int64_t o, const double* coeff, const double* levels,
                 const double* eri_packed, double* eri_mo_packed);
double ao2mo_ump2(Context& cx, Integrals& in, int64_t n, int64_t na, int64_t nb, const double* coeff_a, const double* coeff_b,
                  const double* levels_a, const double* levels_b, const double* eri_packed, double* eri_aa, double* eri_ab, double* eri_bb);
double mo_window(Context& cx, Integrals& in, Solver& sv, int64_t n, int64_t nocc, int64_t nfc, int64_t nfv, const double* levels,
                 const double* eri_mo_packed, double* eri_act);
// E(UMP2) of the three resident blocks (levels on the host, for their basis size), and the blocks themselves for whoever asks
double ump2_of_blocks(Context& cx, const Integrals& in, const double* levels_a, const double* levels_b, int64_t oa, int64_t ob, double* eri_aa,
                      double* eri_ab, double* eri_bb);
// The virtual-virtual block of the MP2 one-particle density from the resident MO integrals (frozen natural orbitals): the
// MP1 amplitude operands are gathered into scratch that goes back to the arena inside the call, D = T~^T T runs through contract(); d_vv
// (v x v, host) comes back symmetric to the bit; returns the frozen-core MP2 energy.  Nothing resident is written.
double mp2_vv_density(Context& cx, const Integrals& in, int64_t n, int64_t nocc, int64_t nfc, const double* levels, double* d_vv);
double ump2_vv_density(Context& cx, const Integrals& in, int64_t n, int64_t na, int64_t nb, int64_t nfc, const double* levels_a,
                       const double* levels_b, double* d_a, double* d_b);
// The frozen-core operator of the active window [nfc, n - nfv) and the core energy from the full MO integrals a transform
// left resident: h_mo = C h_ao C^T through contract(), the core's field gathered by k_core_fold; h_act (n_act x n_act, host) symmetric to
// the bit, *e_core electronic.  Nothing resident is written; the scratch goes back to the arena inside the call.
void core_operator(Context& cx, const Integrals& in, int64_t n, int64_t nfc, int64_t nfv, const double* coeff, const double* h_ao, double* h_act,
                   double* e_core);
void ucore_operator(Context& cx, const Integrals& in, int64_t n, int64_t nfc, int64_t nfv, const double* coeff_a, const double* coeff_b,
                    const double* h_ao, double* h_act_a, double* h_act_b, double* e_core);
// The resident integrals over n_act orbitals as a standard FCIDUMP (fcidump_format.h): compacted on the device, formatted on the host;
// return the number of lines after the header
int64_t write_fcidump_active(Context& cx, const Integrals& in, const char* path, int64_t n_act, int64_t nelec, int64_t ms2, const double* h_act,
                             double e_core_total, double threshold);
int64_t write_fcidump_uactive(Context& cx, const Integrals& in, const char* path, int64_t n_act, int64_t nalpha, int64_t nbeta,
                              const double* h_act_a, const double* h_act_b, double e_core_total, double threshold);
// A standard FCIDUMP as input: fcidump_scan is host only (the header and the number of non-blank lines after it);
// read_fcidump / _uhf parse the file chunk by chunk on the host (fcidump_parse.h), scatter the records on the device into NEW arrays and
// make them resident -- as ao2mo_mp2 / ao2mo_ump2 leave theirs -- only when the whole file was good; every pointer of the result may be
// null and none is written on failure.  Orbitals in file order, the first nocc (nalpha / nbeta) occupied.
struct FcidumpResult {
    double *h[2] = {nullptr, nullptr}, *fock[2] = {nullptr, nullptr}, *levels[2] = {nullptr, nullptr};   // closed shell: [0]; open shell: alpha, beta
    double* eri[3] = {nullptr, nullptr, nullptr};   // packed | aa, bb, ab
    double e_core = 0.0, e_ref = 0.0, fock_offdiag = 0.0;
    double fock_offdiag3[3] = {0.0, 0.0, 0.0};   // read_fcidump_rohf: occupied-occupied, virtual-virtual (off-diagonal), occupied-virtual
    int64_t nread = 0;
};
int fcidump_scan(const char* path, int64_t* norb, int64_t* nelec, int64_t* ms2, int* uhf, int64_t* nlines);
void read_fcidump(Context& cx, Integrals& in, Solver& sv, const char* path, int64_t n, int64_t nocc, FcidumpResult& r);
void read_fcidump_uhf(Context& cx, Integrals& in, const char* path, int64_t n, int64_t na, int64_t nb, FcidumpResult& r);
// a restricted open-shell file (no UHF flag, MS2 = na - nb >= 0): read_fcidump's parse, scatter and residency; r.fock[0] / [1] the two spin
// Fock operators of the determinant (k_fock_ro), r.fock_offdiag3 their largest off-diagonal elements by block
void read_fcidump_rohf(Context& cx, Integrals& in, Solver& sv, const char* path, int64_t n, int64_t na, int64_t nb, FcidumpResult& r);
// The two spin Fock operators of the restricted determinant that fills the first na / nb orbitals (k_fock_ro) for host matrices on the
// resident packed MO array (afesp_mo_fock_ro); returns the electronic reference energy
double mo_fock_ro(Context& cx, const Integrals& in, int64_t n, int64_t na, int64_t nb, const double* h_mo, double* fock_a, double* fock_b);
// The resident packed MO integrals rotated with one orthogonal matrix per spin (new orbital, old orbital) into the three resident blocks
// of the open-shell path, through ao2mo_ump2's transform forms; the packed array and the AO integrals stay as they are
void mo_rotate_uhf(Context& cx, Integrals& in, int64_t n, const double* u_a, const double* u_b, double* eri_aa, double* eri_ab, double* eri_bb);
int64_t read_eri_text(Context& cx, Integrals& in, const char* path, int64_t nbasis, double* eri_packed);
int64_t write_fcidump(Context& cx, const Integrals& in, const char* path, int64_t nbasis);

}  // namespace afesp
