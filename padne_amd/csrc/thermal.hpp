// The thermal handle (thermal.hip) as the translation units that work on it see it: thermal.hip itself, the electro-thermal
// coupling (coupled.hip), which borrows the handle's vertex -> faces lists and its theta, the transient handle
// (transient.hip), coupled_transient.hip, which joins the last two, sdirk.hip, which steps the transient handle by
// error-controlled second-order steps, periodic.hip, which puts states into it for the Krylov iteration on a period, and
// film.hip, which rewrites A's diagonal and hM for a film that depends on the temperature.
#pragma once

#include "error.hpp"

#include <vector>

namespace padne {

// kkt.hip: the V the last padne_kkt_finish_block left on the device, after the checks of every post-processing entry
int kkt_finished_block(const char *entry, padne_ctx *ctx, const padne_kkt *k, int32_t n_cols, const double **V_out, long long *N_out,
                       const padne_csr **L_out);

constexpr int kThermalChunk = 8;       // columns per launch of the load kernel, per step of the face-power kernel (goal.hip's 8)

}  // namespace padne

// the inter-layer coupling of a stacked handle (stack.hip) and the heat sources of a handle (sources.hip), as thermal_sens.hip
// reads them
struct padne_stack {
    int n_layer = 0, n_pair = 0, n_side = 0;
    std::vector<int> mesh_layer, pair_a, pair_b;         // as given
    std::vector<double> pair_g;
    long long n_query = 0, nnz = 0;                      // (side, vertex) slots; stored off-diagonals of G
    std::vector<long long> q_side_off;                   // [n_side + 1] the first slot of every side
    // device (the context's pool).  Slots: owner[q] the global face or -1, vertex[q], weight and cond [q][3]
    int *owner = nullptr, *vertex = nullptr, *mesh_layer_dev = nullptr;
    int *vertex_layer = nullptr;                         // [n_vert] the layer of every vertex (the flows)
    double *weight = nullptr, *cond = nullptr;
    // G without its diagonal as CSR [n_pot], and the diagonal
    int *gptr = nullptr, *gcol = nullptr;
    double *gval = nullptr, *gdiag = nullptr;
};
namespace padne { void stack_free(padne_ctx *ctx, padne_stack *st); }

struct padne_sources {
    int n_source = 0, n_layer = 0;
    long long n_entries = 0;                 // list entries of all sources together
    std::vector<int> layer;                  // per source
    std::vector<long long> lptr_host;        // [n_source + 1]
    // device (the context's pool)
    int *lptr = nullptr, *lface = nullptr;   // source -> faces, ascending
    int *fptr = nullptr, *fsrc = nullptr;    // face -> sources, ascending
    double *A = nullptr;                     // [n_source] A_s
    double *face_area = nullptr;             // [n_tri]
    double *power = nullptr;                 // [power_cols][n_source]
    int power_cols = 0;
};
namespace padne { void sources_free(padne_ctx *ctx, padne_sources *sr); }

// the film curves of a handle (film.hip): the tables, where every vertex row keeps its diagonal, what the create call left
// there and in hM, and the linearisation the next solve uses
struct padne_film {
    std::vector<int> knot_ptr;               // [n_mesh + 1] the first knot of every mesh's table
    std::vector<double> rise, film;          // the knots as given
    // device (the context's pool)
    int *kptr = nullptr;                     // [n_mesh + 1]
    double *krise = nullptr, *kfilm = nullptr, *kslope = nullptr;   // [knots]; kslope[i] the slope of the segment that starts at knot i
    int *diag = nullptr;                     // [n_vert] the entry of A's values that holds the diagonal of the vertex's row
    double *D0 = nullptr, *hM0 = nullptr;    // [n_vert] that diagonal and hM as the create call left them
    double *c = nullptr;                     // [n_vert] what the linearisation adds to the load
    double *lin = nullptr;                   // [n_pot] the iterate the matrix is linearised about
    double *b0 = nullptr;                    // [n_pot] the load of the last solve without c (padne_thermal_resolve)
    bool warm = false;                       // linearised about a held iterate: the next solve starts from lin
    bool have_load = false;                  // b0 holds the load of a solve
};
namespace padne { void film_free(padne_ctx *ctx, padne_film *fm); }

struct padne_thermal {
    padne_ctx *ctx = nullptr;
    const padne_csr *L = nullptr;            // borrowed: the electrical system, for its mesh
    long long n_pot = 0, n_vert = 0, n_tri = 0;
    int n_mesh = 0;
    padne_csr *A = nullptr;                  // owned (with its multigrid hierarchy once a solve has built it)
    int *vptr = nullptr, *vface = nullptr;   // vertex -> incident faces, rows in ascending face order (error_vertex_faces)
    double *Mv = nullptr, *hM = nullptr;     // [n_vert] lumped area and film conductance h_m M_v of every vertex
    std::vector<int64_t> voff, toff;         // the mesh's offset tables on the host
    // of the last solve: face powers [n_cols][n_tri] and temperature rises [n_cols][n_pot], field-major
    double *P = nullptr, *theta = nullptr;
    size_t P_cap = 0, theta_cap = 0;
    int n_cols = 0;
    bool solved = false;
    padne_stack *stack = nullptr;            // owned: the inter-layer coupling of padne_thermal_create_stacked (stack.hip), or null
    padne_sources *sources = nullptr;        // owned: the heat sources of padne_thermal_set_sources (sources.hip), or null
    std::vector<double> film_host;           // [n_mesh] the film coefficients of the create call
    padne_film *film = nullptr;              // owned: the film curves of padne_thermal_set_film_curves (film.hip), or null
};

// The coupling handle (coupled.hip) and the transient handle (transient.hip), as coupled_transient.hip -- which steps the
// one with the scale of the other -- sees them
struct padne_coupled {
    padne_ctx *ctx = nullptr;
    padne_csr *L = nullptr;                  // borrowed: the electrical system, revalued in place
    padne_thermal *th = nullptr;             // borrowed: its lists and its theta
    long long n_vert = 0, n_tri = 0, nnz = 0;
    int n_mesh = 0;
    double *L0 = nullptr;                    // [nnz] the assembled values
    // [n_tri]: the scale of the next revalue, the scale of the last one (what the face kernels use: they belong to the system
    // that was solved), and the face means of the last update
    double *s = nullptr, *s_used = nullptr, *prev = nullptr;
    double *alpha = nullptr;                 // [n_mesh] on the device
    double ambient = 0.0, t0 = 0.0;
    // The lumped resistors whose resistance follows their temperature (padne_coupled_set_resistors), all on the device;
    // n_res 0 without.  [n_res]: the ends, g = 1 / R, alpha and T0, and s, s_used and prev as for the faces
    long long n_res = 0, n_rrow = 0, n_inc = 0;
    int *r_a = nullptr, *r_b = nullptr;
    double *r_g = nullptr, *r_alpha = nullptr, *r_t0 = nullptr;
    double *r_s = nullptr, *r_s_used = nullptr, *r_prev = nullptr;
    // unknown -> resistors: rr_ptr[n_rrow + 1] over the touched rows, and per incidence (resistors ascending within a row)
    // the resistor and the places in L->vals of the row's entry in the other end's column and of its diagonal
    int *rr_ptr = nullptr, *rr_res = nullptr, *rr_other = nullptr, *rr_diag = nullptr;
};

struct padne_transient {
    padne_ctx *ctx = nullptr;
    padne_thermal *th = nullptr;             // borrowed: A, M_v, hM, the vertex -> faces lists, the face powers' array
    long long n_pot = 0, n_vert = 0;
    int n_mesh = 0;
    double *Cv = nullptr;                    // [n_vert]
    padne_csr *S = nullptr;                  // owned: A's pattern (a copy), its own values
    double dt = 0.0;                         // the dt S holds (compared as bits)
    bool have_dt = false;
    double *B = nullptr;                     // [n_case][n_pot]
    int n_case = 0;
    double *theta = nullptr;                 // [n_cols][n_pot]
    double *env = nullptr;                   // [n_cols][n_vert] the largest theta seen ...
    int *env_step = nullptr;                 // ... and the global step that attained it first
    int n_cols = 0;
    bool started = false;
    long long step = 0;                      // steps since the start
    double time = 0.0;                       // their dt, added one by one
    long long hierarchies = 0;               // multigrid setups of S since creation
    // sdirk.hip: the trial step theta_1, theta*, theta_{n+1}, each [n_cols][n_pot] (made by the first trial, dropped with
    // theta when the number of columns changes); live between padne_transient_try_step and whatever ends it
    double *trial[3] = {nullptr, nullptr, nullptr};
    double trial_dt = 0.0;
    bool trial_live = false;
};

namespace padne {

// coupled.hip: the scale kernel and its fold on `theta` (device, null: zeros) -- *d_out (may be null) the largest change of a
// face mean; PADNE_E_INVALID names the lowest face whose scale is invalid.  With resistors set their pass follows: *d_out is
// the larger of the two increments, and the lowest invalid resistor is named when every face is valid
int coupled_run_scale(padne_ctx *ctx, padne_coupled *cp, const double *theta, double *d_out);

// thermal.hip: padne_thermal_solve_kkt with every face's conductance sigma[m] * scale[t] in the place of sigma[m] (scale
// [n_tri] on the device; null: sigma[m] alone, the bits of padne_thermal_solve_kkt)
int thermal_solve_kkt_scaled(const char *entry, padne_ctx *ctx, padne_thermal *th, padne_kkt *plan, int32_t n_cols,
                             const double *scale, int64_t n_heat, const int64_t *heat_node, const int32_t *heat_col,
                             const double *heat_val, const padne_solve_opts *opts, double *theta_host, padne_solve_info *info);

// thermal.hip, for the handles built on a thermal one (transient.hip).  thermal_require: the handle is the context's.
// thermal_check_heat: the checks of the node-heat triples of padne_thermal_solve.  thermal_upload_power: face powers of the
// caller into th->P.  thermal_kkt_block / thermal_kkt_face_power: th->P from the finished block of a plan, in the two halves
// of thermal_solve_kkt_scaled.  thermal_form_load: b[n_cols][n_pot] on the device from th->P[n_cols][n_tri] and the triples.
// thermal_tiles: tiles of 256 items per segment of an offset table
int thermal_require(const char *entry, padne_ctx *ctx, const padne_thermal *th);
int thermal_check_heat(const padne_thermal *th, int32_t n_cols, int64_t n_heat, const int64_t *heat_node, const int32_t *heat_col,
                       const double *heat_val);
int thermal_upload_power(padne_ctx *ctx, padne_thermal *th, int32_t n_cols, const double *face_power_host);
int thermal_kkt_block(const char *entry, padne_ctx *ctx, const padne_thermal *th, padne_kkt *plan, int32_t n_cols,
                      const double **V_out);
int thermal_kkt_face_power(padne_ctx *ctx, padne_thermal *th, int32_t n_cols, const double *V, const double *scale);
int thermal_form_load(padne_ctx *ctx, padne_thermal *th, int32_t n_cols, int64_t n_heat, const int64_t *heat_node,
                      const int32_t *heat_col, const double *heat_val, double *d_b);
std::vector<long long> thermal_tiles(const std::vector<int64_t> &off);
// thermal.hip: the block solve of one or more columns on the face powers th->P, b formed from them and the triples (null
// lists with n_heat 0); film.hip's entries end in it.  thermal_kkt_face_power_column: th->P[1][n_tri] from column `col` of
// the block V[..][ld]
int thermal_solve_core(padne_ctx *ctx, padne_thermal *th, int32_t n_cols, int64_t n_heat, const int64_t *heat_node,
                       const int32_t *heat_col, const double *heat_val, const padne_solve_opts *opts, double *theta_host,
                       padne_solve_info *info, bool resolve = false);
int thermal_kkt_face_power_column(padne_ctx *ctx, padne_thermal *th, int32_t ld, int32_t col, const double *V, const double *scale);
// film.hip, for a handle with film curves.  film_add_load: b[v] = b[v] + c[v] behind thermal_form_load, queued.
// film_refuses: PADNE_E_INVALID for a block of several columns on such a handle
int film_add_load(padne_ctx *ctx, padne_thermal *th, double *d_b);
int film_refuses(const char *entry, const padne_thermal *th, int32_t n_cols);
// sources.hip: what thermal_form_load adds for a handle with heat sources -- their load into b[n_cols][n_pot] on the device,
// queued behind the face gather and the triples; PADNE_E_INVALID without powers for exactly n_cols columns.  Nothing
// without sources
int sources_add_load(padne_ctx *ctx, padne_thermal *th, int32_t n_cols, double *d_b);
// sources.hip: padne_thermal_source_report's sums for any field[n_cols][n_pot] on the device, out_host[n_cols][n_source]
int sources_report_field(padne_ctx *ctx, const padne_thermal *th, int32_t n_cols, const double *field, double *out_host);

// transient.hip, for sdirk.hip.  transient_require: the handle is the context's.  transient_set_dt: S revalued for dt when
// its bits differ from the held ones.  transient_check_cases: case_of_col[n_cols] checked and copied.  transient_opts: the
// defaults of padne_transient_run for null options.  transient_upload_cases: the table on the device, complete on return.
// transient_rhs: the kernel of the step's right-hand side on `theta` [n_cols][n_pot].  TransientPass / transient_pass_init /
// transient_pass: the report kernel and its fold on `theta`, the per-mesh results at out_*[n_cols][n_mesh] on the device;
// the envelope is touched as env_mode says, with `step` as the step that attains
struct TransientPass {
    long long n_vb = 0;
    long long *d_vtile = nullptr, *d_tvert = nullptr;
    double *d_tstored = nullptr, *d_tloss = nullptr, *d_tmax = nullptr;
};
int transient_require(const char *entry, padne_ctx *ctx, const padne_transient *tr);
bool transient_good_dt(double dt);
int transient_set_dt(padne_transient *tr, double dt);
int transient_check_cases(const padne_transient *tr, const int32_t *case_of_col, int n_cols, std::vector<int> *out);
padne_solve_opts transient_opts(const padne_solve_opts *opts);
int transient_upload_cases(padne_transient *tr, Scratch &sc, const std::vector<int> &cases, int **d_case);
int transient_rhs(padne_transient *tr, const int *d_case, double dt, int mode, const double *theta, double *d_rhs);
int transient_pass_init(padne_transient *tr, Scratch &sc, TransientPass *ps);
int transient_pass(padne_transient *tr, const TransientPass &ps, const double *theta, int env_mode, long long step,
                   double *out_stored, double *out_loss, double *out_max, long long *out_vert);
// out[c][p] = theta[c][probe[p]] on the device, queued on the stream
int transient_probe(padne_transient *tr, int n_probe, const long long *d_probe, const double *theta, double *d_out);

// What a matrix derived from its values (1 / diagonal, single-precision copies, multigrid hierarchy) is dropped and rebuilt
// on next use from the values in place; the x-window plan depends on the pattern only and stays
inline void csr_invalidate_values(padne_csr *L) {
    if (L->amg != nullptr) amg_destroy(L->amg);
    L->amg = nullptr;
    if (L->owner != nullptr) {
        pool_free(L->owner, L->dinv);
        pool_free(L->owner, L->vals32);
        pool_free(L->owner, L->dinv32);
    }
    L->dinv = nullptr;
    L->vals32 = nullptr;
    L->dinv32 = nullptr;
}

}  // namespace padne
