/*
 * nvalchemiops_hip.h -- C ABI of libnvalchemiops_hip.so (MI355X / gfx950).
 *
 * Drop-in boundary for the reference's L2 seam: the `torch.library.custom_op` wrappers that launch
 * Warp kernels (reference file:line cited per entry point).  All pointers are DEVICE pointers unless
 * marked [host]; every buffer is owned by the caller (the Python layer allocates through torch's caching
 * allocator, exactly as the reference wrappers do); `stream` is a hipStream_t passed as void*.
 * dtype: 0 = float32, 1 = float64.  Every function returns 0 on success or a negative MI_E* code;
 * mi_last_error() gives a message for the calling thread.
 *
 * State between calls: none that a result depends on.  Three things outlive a call, all documented where they are declared:
 *   - FFT plans (mi_fft_plan_*): explicit handles owned by the caller, each holding its rocFFT work area;
 *   - mi_d3's atom-order heuristic: per device, 64 bytes of pinned host memory with an earlier call's measurement of how spatially
 *     coherent the caller's atom numbering is (it picks between two code paths with bit-identical outputs; see mi_d3);
 *   - the optional per-kernel timing records of mi_timing_enable (bench.py only).
 *
 * A reference maintainer binds these with ctypes; no torch types cross this line.
 */
#ifndef NVALCHEMIOPS_HIP_H
#define NVALCHEMIOPS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI_OK 0
#define MI_EINVAL (-1)   /* bad argument                                   */
#define MI_EHIP (-2)     /* a HIP runtime call failed                      */
#define MI_EWORKSPACE (-3) /* workspace too small                          */
#define MI_ECOMM (-4)    /* RCCL missing, or an RCCL call failed           */

#define MI_F32 0
#define MI_F64 1

/* ---- library ------------------------------------------------------------------------------- */
int mi_version(void);                 /* ABI version, currently 1                                  */
const char* mi_last_error(void);      /* [host] message of the last failure on this thread         */
/* Optional per-kernel timing with HIP events recorded on the launch stream (used by bench.py for the live
 * roofline figure).  mi_timing_report waits for the events and writes "<kernel> <launches> <total_ms>\n" lines. */
int mi_timing_enable(int on);
/* record only the kernel brackets called `name` (NULL / "": all of them): an event record is a packet of its own in the stream, ~5 us of
 * bubble on either side of a kernel, so a timed region that needs ONE kernel's duration selects it and leaves the rest back to back      */
int mi_timing_select(const char* name /*[host]*/);
int mi_timing_report(char* buf /*[host]*/, int cap);
/* same records with per-launch statistics: "<kernel> <launches> <total_ms> <median_ms> <min_ms> <max_ms>\n" */
int mi_timing_report_stats(char* buf /*[host]*/, int cap);
/* HBM calibration streams for the benchmark (no reference counterpart: the reference's protocol, benchmarks/utils.py:133-240, has no
 * in-run calibration): 16-byte-per-lane read / fill / copy streams over caller-owned device buffers, `bytes` a multiple of 16. */
int mi_calibrate_copy(const void* src, void* dst, size_t bytes, void* stream);
int mi_calibrate_fill(void* dst, size_t bytes, float value, void* stream);
int mi_calibrate_read(const void* src, size_t bytes, float* sink /* 1 float, never written in practice */, void* stream);

/* ---- neighbour list -------------------------------------------------------------------------
 * Replaces: nvalchemiops::build_cell_list + ::query_cell_list (neighborlist/cell_list.py:725,892),
 * ::batch_build_cell_list + ::batch_query_cell_list (batch_cell_list.py:739,915), the padded-matrix
 * fill of cell_list()/batch_cell_list() (cell_list.py:1358-1373), the naive ops (naive.py:221,299) and
 * get_neighbor_list_from_neighbor_matrix (neighbor_utils.py:362-441).
 *
 * One fused pipeline: per-system grid setup -> cell keys -> radix sort by cell -> cell ranges ->
 * cell-ordered position copy -> wave64-per-atom full-shell query with ballot/popcount compaction.
 * Rows are written only by their owner wave (no atomics, deterministic order), padding included.
 */
#define MI_NL_MODE_MATRIX 0   /* write neighbor_matrix / shifts / num_neighbors (+ padding)          */
#define MI_NL_MODE_COUNT 1    /* write num_neighbors only (first pass of direct CSR emission)        */
#define MI_NL_MODE_CSR 2      /* write list_ij / list_shifts at neighbor_ptr[i] (second pass)         */

#define MI_NL_HALF_FILL 1     /* keep one of (i,j,S)/(j,i,-S): S lexicographically > 0, or S==0 and j>i */
#define MI_NL_NAIVE_EXPR 2    /* distance expression / cutoff^2 rounding / image range of naive.py:37-182 */
#define MI_NL_REUSE_GRID 4    /* skip the binning stages: workspace still holds the grid of the previous call */
#define MI_NL_NO_SHIFTS 8     /* matrix mode: do not write the shifts tensor (non-periodic naive output)  */
#define MI_NL_NO_PAD 16       /* matrix mode: leave slots >= num_neighbors untouched (query_cell_list: the
                                 caller pre-filled the outputs, cell_list.py:892-1034)                    */

size_t mi_nl_workspace_bytes(int n_atoms, int n_systems, int dtype);

int mi_nl_neighbors(const void* positions,          /* [n_atoms,3] dtype                              */
                    int n_atoms,
                    const void* cell,               /* [n_systems,3,3] dtype, rows = lattice vectors   */
                    const uint8_t* pbc,             /* [n_systems,3] bool                              */
                    const int32_t* batch_idx,       /* [n_atoms] or NULL (single system)               */
                    int n_systems, double cutoff, int dtype, int mode, int flags,
                    int32_t* neighbor_matrix,       /* [n_atoms,max_neighbors]      (MATRIX)           */
                    int32_t* neighbor_matrix_shifts,/* [n_atoms,max_neighbors,3]    (MATRIX)           */
                    int32_t* num_neighbors,         /* [n_atoms]                    (MATRIX, COUNT)    */
                    int max_neighbors, int fill_value,
                    const int32_t* neighbor_ptr,    /* [n_atoms+1]                  (CSR)              */
                    int32_t* list_ij,               /* [2,n_pairs]                  (CSR)              */
                    int32_t* list_shifts,           /* [n_pairs,3]                  (CSR)              */
                    long long n_pairs,
                    const void* bin_origin,         /* [n_systems,3] dtype or NULL: origin subtracted for BINNING
                                                       only (non-periodic inputs far from 0); distances use the
                                                       caller's coordinates unchanged                        */
                    void* workspace, size_t workspace_bytes, void* stream);

/* Matrix-mode search that also leaves a PACKED COMPANION of the padded matrix (round 5): one 32-bit word per slot -- neighbour index in
 * bits 0-25, unit shift + 1 in three 2-bit fields (bits 26-31), 0xffffffff = padding -- behind a 256-byte header whose first int32 is
 * raised (non-zero) when a stored shift lies outside {-1, 0, 1} (the companion is then unusable).  It is the format the D3 passes stream
 * (mi_d3_packed below): the search has index and shift of every hit in registers when it stores the 16 bytes of the API format, so the
 * 4-byte word costs one more store there and saves the consumer a 16 B/slot read + 4 B/slot write.  No reference counterpart: the
 * reference's dftd3 kernels re-read neighbor_matrix + neighbor_matrix_shifts in every pass (dftd3.py:833-1260).  The companion describes
 * exactly what was written to neighbor_matrix / neighbor_matrix_shifts by THIS call; keeping the two in step afterwards is the caller's
 * business (the Python layer keys it on the tensors' version counters).  Requires shifts, padding, a full (not half-filled) list and
 * n_atoms < 2^26.  packed_out: mi_nl_packed_bytes(n_atoms, max_neighbors) bytes (0 = not available for these sizes).                    */
size_t mi_nl_packed_bytes(int n_atoms, int max_neighbors);
int mi_nl_neighbors_packed(const void* positions, int n_atoms, const void* cell, const uint8_t* pbc, const int32_t* batch_idx, int n_systems,
                           double cutoff, int dtype, int flags, int32_t* neighbor_matrix, int32_t* neighbor_matrix_shifts,
                           int32_t* num_neighbors, int max_neighbors, int fill_value, const void* bin_origin, void* workspace,
                           size_t workspace_bytes, void* packed_out, size_t packed_bytes, void* stream);

/* mi_nl_neighbors_packed that ALSO sums the DFT-D3 coordination numbers of the list it writes (round 6):
 *   CN_i = sum over the stored entries (j, S) of row i of 1 / (1 + exp(-k1 ((rcov[Z_i] + rcov[Z_j]) / |r_j - r_i + S.cell| - 1)))
 * -- what the reference's first D3 pass computes by walking the whole list again (`_cn_kernel_nm`, interactions/dispersion/dftd3.py:833-941,
 * `_cn_counting` :608-645).  The search has the squared distance of every hit in registers and both atoms' records in LDS, so the sum is a
 * handful of instructions inside a kernel that waits for its stores; mi_d3_packed_cn below then skips its CN pass.  Atoms with Z <= 0 or
 * Z >= nz take part in the search but neither have nor contribute a coordination number (dftd3.py:871-885).
 * cn_out: mi_nl_cn_bytes(n_atoms) bytes = a 1 KiB header + float cn[n_atoms] (caller's atom order).  Header: int32[0] is raised when the
 * numbers must not be used (a row overflowed max_neighbors: the stored list's own sum is smaller); float[2] = cutoff, float[3] = k1 log2(e);
 * 64 uint64 checksum slots at byte 256 whose wrapping sum fingerprints the inputs the numbers were computed from (every atom's index,
 * system, position bits and covalent radius, the cell, k1).  mi_d3_packed_cn recomputes the fingerprint from ITS inputs on the device and
 * only adopts the numbers on a match, so a consumer called with other positions (an MD step that reuses the list), other species or
 * another cell silently runs its own pass -- there is no host-side bookkeeping to get wrong.
 * `request` is read on the host; its pointers are device pointers.  Not combinable with MI_NL_REUSE_GRID / half-fill.                    */
typedef struct mi_nl_cn_request {
  const int32_t* numbers;       /* [n_atoms] atomic numbers                                   */
  const float* covalent_radii;  /* [nz] fp32, index 0 = padding (D3Parameters.rcov as fp32)    */
  int nz;
  float k1;                     /* steepness of the counting function (dftd3 default 16)       */
} mi_nl_cn_request;
size_t mi_nl_cn_bytes(int n_atoms);
int mi_nl_neighbors_packed_cn(const void* positions, int n_atoms, const void* cell, const uint8_t* pbc, const int32_t* batch_idx, int n_systems,
                              double cutoff, int dtype, int flags, int32_t* neighbor_matrix, int32_t* neighbor_matrix_shifts,
                              int32_t* num_neighbors, int max_neighbors, int fill_value, const void* bin_origin, void* workspace,
                              size_t workspace_bytes, void* packed_out, size_t packed_bytes, const mi_nl_cn_request* request /* [host] */,
                              void* cn_out, size_t cn_bytes, void* stream);

/* Single-sweep dual-cutoff search: ONE walk over the candidate pairs fills two padded matrices, the short list nested in the long one and
 * both with the image range of the long cutoff.  Replaces: _fill_naive_neighbor_matrix[_pbc]_dual_cutoff and the batch variants
 * (neighborlist/naive_dual_cutoff.py:36,115 / batch_naive_dual_cutoff.py:37,126).  flags as for mi_nl_neighbors (matrix mode). */
int mi_nl_neighbors_dual(const void* positions, int n_atoms, const void* cell, const uint8_t* pbc, const int32_t* batch_idx, int n_systems,
                         double cutoff_short, double cutoff_long, int dtype, int flags,
                         int32_t* neighbor_matrix_short, int32_t* neighbor_matrix_shifts_short, int32_t* num_neighbors_short,
                         int max_neighbors_short,
                         int32_t* neighbor_matrix_long, int32_t* neighbor_matrix_shifts_long, int32_t* num_neighbors_long,
                         int max_neighbors_long, int fill_value, const void* bin_origin, void* workspace, size_t workspace_bytes,
                         void* stream);

/* padded matrix -> COO/CSR (neighbor_utils.py:362-441): entries != fill_value, row-major.
 * neighbor_ptr = [0, cumsum(num_neighbors)] supplied by the caller; shifts may be NULL.              */
int mi_nl_matrix_to_coo(const int32_t* neighbor_matrix, const int32_t* neighbor_matrix_shifts,
                        const int32_t* neighbor_ptr, int n_atoms, int max_neighbors, int fill_value,
                        int32_t* list_ij, int32_t* list_shifts, long long n_pairs, void* stream);

/* Reference-format cell-list cache (cell_list.py:725-889 / batch_cell_list.py:739-912): fills
 * cells_per_dimension, atom_periodic_shifts, atom_to_cell_mapping, atoms_per_cell_count,
 * cell_atom_start_indices, cell_atom_list with the reference's binning rule for `max_total_cells`
 * cells (atoms inside a cell are listed in ascending index order).                                   */
int mi_nl_build_cell_cache(const void* positions, int n_atoms, const void* cell, const uint8_t* pbc,
                           const int32_t* batch_idx, int n_systems, double cutoff, int dtype,
                           int max_total_cells, int32_t* cells_per_dimension, int32_t* atom_periodic_shifts,
                           int32_t* atom_to_cell_mapping, int32_t* atoms_per_cell_count,
                           int32_t* cell_atom_start_indices, int32_t* cell_atom_list, void* workspace,
                           size_t workspace_bytes, void* stream);

/* estimate_cell_list_sizes kernels (cell_list.py:35-99 / batch_cell_list.py:36-99)                   */
int mi_nl_estimate_sizes(const void* cell, const uint8_t* pbc, int n_systems, double cutoff, int max_nbins,
                         int dtype, int32_t* number_of_cells /*[n_systems]*/,
                         int32_t* neighbor_search_radius /*[n_systems,3]*/, void* stream);

/* Bounding boxes of non-periodic systems: cell_out[s] = diag(max(hi - lo, 1) * 1.001), origin_out[s] = lo, the binning frame a
 * free-space search uses when the caller gives no cell (reference: `neighbor_list` fabricates a unit cell, neighborlist.py:220-226;
 * SURVEY Appendix B.2).  `scratch`: 6 * n_systems 8-byte words.  batch_idx NULL = one system.                               */
int mi_nl_bounding_cells(const void* positions, const int32_t* batch_idx, int n_atoms, int n_systems, int dtype, void* cell_out,
                         void* origin_out, void* scratch, void* stream);

/* Rebuild detection for MD loops (neighborlist/rebuild_detection.py:37-170): `flag` (one byte, zeroed by the caller)
 * is set when any atom's cell (reference binning of mi_nl_build_cell_cache) differs from atom_to_cell_mapping, resp. when any atom
 * moved farther than `threshold` from its reference position.                                                                    */
int mi_nl_cells_changed(const void* positions, const void* cell /*[3,3]*/, const int32_t* atom_to_cell_mapping,
                        const int32_t* cells_per_dimension /*[3]*/, const uint8_t* pbc /*[3]*/, int n_atoms, int dtype,
                        uint8_t* flag, void* stream);
int mi_nl_moved_beyond_skin(const void* reference_positions, const void* current_positions, double threshold, int n_atoms, int dtype,
                            uint8_t* flag, void* stream);

/* ---- DFT-D3(BJ) -----------------------------------------------------------------------------
 * Replaces nvalchemiops::dftd3_nm (dftd3.py:1792-2122) and ::dftd3_nl (:2125-2465): CN pass, fused
 * C6-interpolation + BJ damping + energy + direct force + dE/dCN pass, chain-rule force pass.  The
 * reference's pass 0 (materialised cartesian_shifts) is folded into the passes.  Outputs are float32
 * whatever `dtype` (the positions/cell dtype) is.  Layout selector: neighbor_ptr == NULL -> padded matrix
 * (entries >= fill_value are padding), else CSR (idx_j[neighbor_ptr[i]..neighbor_ptr[i+1])).
 * Atoms with Z <= 0 or Z >= nz are padding, as a neighbour and as the owner of a row: part of no pair and of no coordination number, no
 * table entry is read for them, and their force and coordination number are 0 (mi_d3, mi_d3_zero, mi_d3_atm, mi_d3_zero_atm alike).
 */
typedef struct {
  const float* rcov;   /* [nz]            */
  const float* r4r2;   /* [nz]            */
  const float* c6ab;   /* [nz,nz,5,5]     */
  const float* cn_ref; /* [nz,nz,5,5]     */
  int nz;              /* max_Z + 1       */
  float a1, a2, s6, s8, k1, k3, s5_on, s5_off;
} mi_d3_params;

size_t mi_d3_workspace_bytes(int n_atoms, int n_systems, int nz);
/* Optional larger workspace for a periodic padded matrix: base + 4 bytes per slot.  Given at least this much, mi_d3 lets its CN pass
 * leave a packed copy of the list (index + unit shift in one word) that the energy and chain passes stream instead of the caller's
 * 16-byte-per-slot arrays; lists with shifts outside {-1,0,1} or >= 2^26 atoms fall back to the arrays on the device. Results are
 * identical either way.  Equals mi_d3_workspace_bytes when max_neighbors <= 0 (CSR).                                              */
size_t mi_d3_workspace_bytes_packed(int n_atoms, int n_systems, int nz, int max_neighbors);
/* The same for any layout, by number of stored entries (CSR: neighbor_ptr[n_atoms] = mi_d3's `n_list_entries`).              */
size_t mi_d3_workspace_bytes_entries(int n_atoms, int n_systems, int nz, long long n_entries);

/* Atom-order heuristic (the one thing mi_d3 remembers between calls): with the packed list and >= 2048 atoms the passes can walk spatially
 * ordered copies of the per-atom records, which pays when the caller numbers its atoms incoherently and costs a little when it does not.
 * The choice is made on the host from a measurement an EARLIER call left in pinned host memory (asynchronous copy, no synchronisation,
 * records kept per device and per (n_atoms, n_systems) generation); both paths produce bit-identical outputs, so the state can change
 * run-to-run timing only.  Nothing is measured or published while `stream` is being captured into a HIP graph: the choice made at capture
 * time is part of the graph.  NVALCHEMIOPS_D3_SORT=0|1 in the environment forces the choice.                                         */
int mi_d3(const void* positions, const int32_t* numbers, int n_atoms, int dtype,
          const int32_t* idx_j,        /* matrix [n_atoms,max_neighbors] or CSR values [n_pairs]      */
          const int32_t* unit_shifts,  /* same layout x3, or NULL (non-periodic)                      */
          const int32_t* neighbor_ptr, /* NULL => matrix layout                                       */
          int max_neighbors,           /* matrix row width (ignored for CSR)                          */
          long long n_list_entries,    /* CSR: length of idx_j, 0 = unknown (no packed copy); ignored for the matrix layout */
          int fill_value,
          const void* cell,            /* [n_systems,3,3] dtype or NULL                               */
          const int32_t* batch_idx,    /* [n_atoms] or NULL                                           */
          int n_systems, const mi_d3_params* params /* [host] */, int compute_virial,
          float* energy /*[n_systems]*/, float* forces /*[n_atoms,3]*/, float* coord_num /*[n_atoms]*/,
          float* virial /*[n_systems,3,3] or NULL*/, void* workspace, size_t workspace_bytes, void* stream);

/* mi_d3 on a periodic padded matrix whose packed companion the search already wrote (mi_nl_neighbors_packed): the CN pass streams the
 * 4 B/slot companion instead of the 16 B/slot arrays and writes no copy of its own; the energy and chain passes read the companion too.
 * neighbor_matrix / neighbor_matrix_shifts must still be the arrays the companion was built with: they are what the passes read when the
 * companion's flag is raised (device-side choice, no host round trip), and the results are bit-identical to mi_d3's either way.
 * `workspace` as for mi_d3 (with mi_d3_workspace_bytes_packed's size the spatial order stays available for incoherently numbered atoms).
 * Requires cell, shifts, fill_value >= n_atoms, n_atoms < 2^26.                                                                          */
int mi_d3_packed(const void* positions, const int32_t* numbers, int n_atoms, int dtype, const int32_t* neighbor_matrix,
                 const int32_t* neighbor_matrix_shifts, int max_neighbors, int fill_value, const void* cell, const int32_t* batch_idx,
                 int n_systems, const mi_d3_params* params, int compute_virial, float* energy, float* forces, float* coord_num, float* virial,
                 void* workspace, size_t workspace_bytes, const void* packed_list, size_t packed_bytes /* >= mi_nl_packed_bytes(...) */,
                 void* stream);

/* mi_d3_packed with two additions (round 6):
 *  - `cn_block` (optional, NULL = none): the coordination numbers the search summed while it wrote the list (mi_nl_neighbors_packed_cn).
 *    They are adopted -- and the CN pass skipped -- iff the block's flag is clear AND the fingerprint in its header equals the one this call
 *    computes on the device from its own positions, numbers, params->rcov, params->k1, cell and batch_idx; otherwise the CN pass runs as in
 *    mi_d3_packed.  Either way coord_num is the reference's sum over the stored list to fp32 rounding (the two evaluations differ in
 *    summation order and in one rounding of the exponent: <= 1e-6 relative, tests/test_search_cn_gpu.py).
 *  - a sampled consistency check of the companion against the arrays it claims to describe: one row in every block of `verify_stride`
 *    consecutive rows (at offset (verify_phase + hash(block)) mod verify_stride: consecutive phases visit every row once in verify_stride
 *    calls, and no regular edit pattern can hide between the samples) is re-derived from neighbor_matrix / neighbor_matrix_shifts and
 *    compared word by word; on a
 *    mismatch the call falls back to the 16 B/slot arrays (device-side flag, no host round trip, results = mi_d3's on the arrays as they
 *    are NOW).  verify_stride = 1 checks every row, 0 disables the check (mi_d3_packed itself uses stride 64, phase 0).  This catches
 *    arrays edited behind the companion's back in bulk (a filtering kernel, a copy from elsewhere); a single edited entry in an unsampled
 *    row is not seen -- callers who edit lists through raw pointers must drop the companion.                                           */
int mi_d3_packed_cn(const void* positions, const int32_t* numbers, int n_atoms, int dtype, const int32_t* neighbor_matrix,
                    const int32_t* neighbor_matrix_shifts, int max_neighbors, int fill_value, const void* cell, const int32_t* batch_idx,
                    int n_systems, const mi_d3_params* params, int compute_virial, float* energy, float* forces, float* coord_num, float* virial,
                    void* workspace, size_t workspace_bytes, const void* packed_list, size_t packed_bytes, const void* cn_block, size_t cn_bytes,
                    int verify_stride, int verify_phase, void* stream);

/* ---- DFT-D3 with zero damping: D3(0) and D3M(0) ----------------------------------------------------
 * No reference counterpart (its dftd3 has the BJ damping only).  mi_d3 with the damping function of the original D3 parametrisation:
 *   E_ij = -C6_ij(CN_i, CN_j) [s6 f_6(r) / r^6 + s8 q f_8(r) / r^8] sw(r),   q = 3 r4r2_i r4r2_j,
 *   f_n(r) = 1 / (1 + 6 (r / (rs_n R0) + beta R0)^(-alpha_n)),   alpha_6 = alpha, alpha_8 = alpha + 2,   R0 = r0ab[Z_i, Z_j]
 * (beta = 0: D3(0); beta != 0: the modified form D3M(0)).  Everything else -- the coordination numbers, the C6 interpolation, the 1/2 per
 * stored directed pair, the c6 < 1e-12 skip, the s5 switch, forces including the path through the coordination numbers, the virial, the
 * outputs and the workspace (mi_d3_workspace_bytes*: the species-pair constants reuse the room the BJ ones take) -- is mi_d3's.
 * params->a1 / a2 are ignored.  r0ab is the symmetric [nz,nz] table of pair cutoff radii in Bohr (device memory, float32; row / column 0
 * is padding); a pair whose entry is <= 0 contributes nothing (energy, force, virial and dE/dCN are zero for it).  alpha == 14 takes the
 * powers by repeated squaring, any other exponent one log2 / exp2 pair per power.  A close contact (x^-alpha overflowing fp32) gives f = 0
 * and a zero derivative, not a NaN.  Requires rs6 > 0, rs8 > 0, alpha > 0.                                                               */
typedef struct {
  float rs6, rs8, alpha, beta;
  const float* r0ab; /* [nz,nz] */
} mi_d3_zero_params;

int mi_d3_zero(const void* positions, const int32_t* numbers, int n_atoms, int dtype, const int32_t* idx_j, const int32_t* unit_shifts,
               const int32_t* neighbor_ptr, int max_neighbors, long long n_list_entries, int fill_value, const void* cell,
               const int32_t* batch_idx, int n_systems, const mi_d3_params* params /* [host] */, const mi_d3_zero_params* zero /* [host] */,
               int compute_virial, float* energy, float* forces, float* coord_num, float* virial, void* workspace, size_t workspace_bytes,
               void* stream);

/* mi_d3_packed_cn (companion, adoption of the search's coordination numbers, sampled check: all as described there) with zero damping.  */
int mi_d3_zero_packed_cn(const void* positions, const int32_t* numbers, int n_atoms, int dtype, const int32_t* neighbor_matrix,
                         const int32_t* neighbor_matrix_shifts, int max_neighbors, int fill_value, const void* cell, const int32_t* batch_idx,
                         int n_systems, const mi_d3_params* params, const mi_d3_zero_params* zero, int compute_virial, float* energy,
                         float* forces, float* coord_num, float* virial, void* workspace, size_t workspace_bytes, const void* packed_list,
                         size_t packed_bytes, const void* cn_block, size_t cn_bytes, int verify_stride, int verify_phase, void* stream);

/* ---- DFT-D3 three-body (Axilrod-Teller-Muto) term --------------------------------------------------
 * No reference counterpart (its dftd3 is two-body only).  For every unordered triple of distinct atom images A, B, C whose three distances
 * are all < three_body_cutoff:  E_ABC = s9 sqrt(C6_AB C6_AC C6_BC) ang fdamp,  ang = (3 cosA cosB cosC + 1) / (r_AB r_AC r_BC)^3,
 * fdamp = 1 / (1 + 6 (R0_AB R0_AC R0_BC / (r_AB r_AC r_BC))^(alpha / 3)),  R0_XY = a1 sqrt(3 r4r2_X r4r2_Y) + a2,  C6_XY = mi_d3's own
 * interpolation with mi_d3's coordination numbers (summed over ALL stored entries of the list).  Outputs are the three-body contribution
 * alone, in mi_d3's units, dtypes and virial convention, so they add to mi_d3's: energy per system (each triple once per unit cell),
 * forces = -dE/dr including the path through the coordination numbers, virial.  params->s6 / s8 / s5_* are not used.
 * The list (either layout, as for mi_d3) must be a FULL list (every pair stored in both rows) with a cutoff >= three_body_cutoff; entries
 * beyond three_body_cutoff only count for the coordination numbers.  Reads the caller's arrays: there is no packed-companion variant.
 * After the call the n_atoms uint32 at byte mi_d3_atm_visits_offset(...) of the workspace hold, per centre atom, the number of triangles
 * visited from it (each triangle is visited from its three vertices; a diagnostic for benchmarks).  mi_d3_atm_tile(): neighbours inside
 * three_body_cutoff a row may have before the triple pass works tile by tile (results do not depend on it).                              */
size_t mi_d3_atm_workspace_bytes(int n_atoms, int n_systems, int nz);
size_t mi_d3_atm_visits_offset(int n_atoms, int n_systems, int nz);
int mi_d3_atm_tile(void);
int mi_d3_atm(const void* positions, const int32_t* numbers, int n_atoms, int dtype,
              const int32_t* idx_j, const int32_t* unit_shifts, const int32_t* neighbor_ptr /* NULL => matrix layout */,
              int max_neighbors, int fill_value, const void* cell, const int32_t* batch_idx, int n_systems,
              const mi_d3_params* params /* [host] */, float s9, float alpha, float three_body_cutoff, int compute_virial,
              float* energy /*[n_systems]*/, float* forces /*[n_atoms,3]*/, float* virial /*[n_systems,3,3] or NULL*/,
              void* workspace, size_t workspace_bytes, void* stream);

/* mi_d3_atm with the radii zero damping conventionally pairs it with: R0_XY = rs9 r0ab[Z_X, Z_Y] (rs9 = 4/3 by convention; r0ab as for
 * mi_d3_zero: symmetric [nz,nz], Bohr, device memory, float32) instead of a1 sqrt(3 r4r2_X r4r2_Y) + a2.  params->a1 / a2 are ignored.  A
 * triple with a pair whose r0ab entry is <= 0 contributes nothing.  Everything else -- arguments, outputs, list requirements, workspace
 * (mi_d3_atm_workspace_bytes), the visit counters -- is mi_d3_atm's.  Requires rs9 > 0.                                                 */
int mi_d3_zero_atm(const void* positions, const int32_t* numbers, int n_atoms, int dtype,
                   const int32_t* idx_j, const int32_t* unit_shifts, const int32_t* neighbor_ptr /* NULL => matrix layout */,
                   int max_neighbors, int fill_value, const void* cell, const int32_t* batch_idx, int n_systems,
                   const mi_d3_params* params /* [host] */, float s9, float alpha, float three_body_cutoff, float rs9,
                   const float* r0ab /* [nz,nz] */, int compute_virial, float* energy, float* forces, float* virial,
                   void* workspace, size_t workspace_bytes, void* stream);

/* ---- DFT-D4 two-body dispersion (csrc/d4.hip) -------------------------------------------------------------------------------------
 * No reference counterpart.  The D4 two-body energy with Becke-Johnson damping and a C6 that depends on each atom's coordination number
 * AND partial charge, over the entries (i, j, S) of a FULL list in either layout of mi_d3 (r = r_j - r_i + S . cell).  Tables are indexed
 * by Z (index 0 = padding), element Z has n_ref[Z] <= 7 references a with cn_ref[Z,a], q_ref[Z,a], ngw[Z,a] in {1,2,3}:
 *   CN_i    = sum_row delta(Z_i,Z_j) 1/2 (1 + erf(-k_cn (r / (rcov_i + rcov_j) - 1))),  delta = k4 exp(-(|en_i - en_j| + k5)^2 / k6);
 *             with cn_cutoff > 0 entries with r >= cn_cutoff do not count (hard cut), cn_cutoff <= 0: every stored entry counts
 *   g_a     = sum_{s=1..ngw_a} exp(-wf s (CN_i - cn_ref_a)^2),   W_a = g_a / sum_b g_b          (evaluated max-shifted: never 0/0)
 *   zeta_a  = exp(ga (1 - exp(gc gam[Z] (1 - (zeff[Z] + q_ref_a) / (zeff[Z] + q_i)))))   if zeff[Z] + q_i > 0,  else exp(ga)
 *   w_i[a]  = W_a zeta_a,   C6_ij = sum_ab w_i[a] c6_ref[Z_i,Z_j,a,b] w_j[b]              (c6_ref[A,B,a,b] = c6_ref[B,A,b,a] is required)
 *   E       = 1/2 sum_entries -C6_ij (s6 / (r^6 + R0^6) + s8 Q / (r^8 + R0^8)),   Q = 3 r4r2_i r4r2_j,  R0 = a1 sqrt(Q) + a2
 * Table entries with reference index >= n_ref[Z] are never used, whatever they hold.  Atoms with Z <= 0, Z >= nz or n_ref[Z] = 0 are
 * padding: part of no pair and of no CN, their force, CN and dE/dq are 0.  Entries with r <= 1e-8 contribute nothing.
 * Outputs (float32 whatever `dtype`): energy per system, forces at fixed charges including the path through the coordination numbers,
 * coord_num, charge_grad = dE/dq_i, virial = -dE/d(strain) (needs cell and unit_shifts).  No atomics: two identical calls give
 * bit-identical outputs.  mi_d4_species_slots(): distinct species of one call whose contracted C6 vectors a wave holds in LDS at once;
 * with more species present a row is walked once per group of that many (same results).  mi_d4_fold_blocks(): blocks of 256 threads per
 * system in the fixed-order fold of the per-row energies and virials (mi_d4 and mi_d4_atm): a block takes the rows
 * x*256 + t + k*256*mi_d4_fold_blocks(), so systems beyond 256*mi_d4_fold_blocks() atoms make a second trip.  n_list_entries is accepted
 * for symmetry with mi_d3 and not read.                                                                                                 */
typedef struct {
  const float* rcov;     /* [nz]          used as given                     */
  const float* en;       /* [nz]          electronegativities               */
  const float* r4r2;     /* [nz]                                            */
  const float* zeff;     /* [nz]          effective nuclear charges         */
  const float* gam;      /* [nz]          chemical hardnesses               */
  const int32_t* n_ref;  /* [nz]          references per element, 0 ... 7   */
  const int32_t* ngw;    /* [nz,7]        Gaussian weights per reference    */
  const float* cn_ref;   /* [nz,7]                                          */
  const float* q_ref;    /* [nz,7]                                          */
  const float* c6_ref;   /* [nz,nz,7,7]                                     */
  int nz;                /* max_Z + 1                                       */
  float a1, a2, s6, s8, k_cn, k4, k5, k6, wf, ga, gc;
  float cn_cutoff;       /* <= 0: none                                      */
} mi_d4_params;
size_t mi_d4_workspace_bytes(int n_atoms, int n_systems, int nz);
int mi_d4_species_slots(void);
int mi_d4_fold_blocks(void);
int mi_d4(const void* positions, const int32_t* numbers, int n_atoms, int dtype, const int32_t* idx_j, const int32_t* unit_shifts,
          const int32_t* neighbor_ptr /* NULL => matrix layout */, int max_neighbors, long long n_list_entries, int fill_value,
          const void* cell, const int32_t* batch_idx, int n_systems, const mi_d4_params* params /* [host] */,
          const float* charges /* [n_atoms] */, int compute_virial, float* energy /*[n_systems]*/, float* forces /*[n_atoms,3]*/,
          float* coord_num /*[n_atoms]*/, float* charge_grad /*[n_atoms]*/, float* virial /*[n_systems,3,3] or NULL*/,
          void* workspace, size_t workspace_bytes, void* stream);

/* ---- DFT-D4 three-body (Axilrod-Teller-Muto) term (csrc/d4_atm.h) --------------------------------------------------------------------
 * No reference counterpart.  For every unordered triple of distinct atom images A, B, C whose three distances are all
 * < three_body_cutoff:
 *   E_ABC  = s9 sqrt(C6_AB C6_AC C6_BC) ang fdamp
 *   ang    = 0.375 (a + b - c)(a + c - b)(b + c - a) / P^5 + 1 / P^3        a, b, c squared sides, P product of the sides
 *   fdamp  = 1 / (1 + 6 (R0_AB R0_AC R0_BC / P)^(alpha / 3)),               R0_XY = a1 sqrt(3 r4r2_X r4r2_Y) + a2
 *   C6_XY  = sum_ab w_X[a] c6_ref[Z_X,Z_Y,a,b] w_Y[b],                      w_X[a] = W_a(CN_X) zeta_a(q = 0)
 * W_a, zeta_a, the coordination number (erf count, electronegativity factor, optional hard cn_cutoff) and the padding rules (Z <= 0,
 * Z >= nz, n_ref[Z] = 0; table entries beyond n_ref are never read) are exactly mi_d4's.  The charge scaling is evaluated at q = 0 for
 * every atom -- D4's definition of the term -- so there is no charges argument and no dE/dq output; zeta_a(0) is not 1: it depends on q_ref,
 * zeff, gam, ga and gc.  CN is summed over ALL stored entries of the list (subject to cn_cutoff); entries beyond three_body_cutoff only
 * count for CN.  A triple with any C6 < 1e-12 contributes nothing.  Each triple counts once per unit cell.
 * Outputs are the three-body contribution alone, float32, to be ADDED to mi_d4's: energy per system, forces = -dE/dr including the path
 * through the coordination numbers, virial in mi_d4's convention (needs cell and unit_shifts).  params->s6 / s8 are not used.  The list
 * (either layout) must be a FULL list with a cutoff >= three_body_cutoff.  No atomics: two identical calls give bit-identical outputs.
 * Requires finite three_body_cutoff > 0, alpha > 0 and s9.  After the call the n_atoms uint32 at byte mi_d4_atm_visits_offset(...) of the
 * workspace hold, per centre atom, the number of triangles visited from it (each triangle is visited from its three vertices; a diagnostic
 * for benchmarks).  mi_d4_atm_tile(): neighbours inside three_body_cutoff a row may have before the triple pass works tile by tile
 * (results do not depend on it).  More species in one call than mi_d4_species_slots(): same results, slower.                            */
size_t mi_d4_atm_workspace_bytes(int n_atoms, int n_systems, int nz);
size_t mi_d4_atm_visits_offset(int n_atoms, int n_systems, int nz);
int mi_d4_atm_tile(void);
int mi_d4_atm(const void* positions, const int32_t* numbers, int n_atoms, int dtype, const int32_t* idx_j, const int32_t* unit_shifts,
              const int32_t* neighbor_ptr /* NULL => matrix layout */, int max_neighbors, int fill_value, const void* cell,
              const int32_t* batch_idx, int n_systems, const mi_d4_params* params /* [host] */, float s9, float alpha,
              float three_body_cutoff, int compute_virial, float* energy /*[n_systems]*/, float* forces /*[n_atoms,3]*/,
              float* virial /*[n_systems,3,3] or NULL*/, void* workspace, size_t workspace_bytes, void* stream);

/* ---- Ewald real space -----------------------------------------------------------------------
 * Replaces the 12 alchemiops::_[batch_]ewald_real_space_* ops (ewald.py:263-1365; kernels
 * ewald_kernels.py:266-1495): erfc(A&S 7.1.26)-damped pair sum over the stored neighbour entries.
 * energies are float64 whatever dtype is (the wrapper casts, ewald.py:577).  The reference adds -f to atom i and
 * atomically +f to atom j for every stored entry (ewald_kernels.py:518-544; charge gradients :864-873).  Over a
 * symmetric (full) list that is 2x the row owner's sum, which is what the fast path writes (no atomics).
 * `scratch` (device memory, may be NULL) has two optional parts, used when `scratch_bytes` covers them:
 *   [0, mi_ewald_symmetry_scratch_bytes())            list-symmetry checksums: when given, the same pass checksums the list in both
 * directions and, if it is NOT symmetric (half lists, rows truncated by overflow, one-sided lists), two fix-up launches
 * redo forces / charge gradients with the reference's scatter; they exit at once otherwise.  Without it the caller
 * guarantees a symmetric list.
 *   [.., mi_ewald_real_scratch_bytes(n_atoms, dtype))  {x,y,z,q} records: the pair loop then gathers one record per neighbour
 *                                                      instead of three coordinates + the charge (same arithmetic, same results).
 */
#define MI_EW_FORCES 1
#define MI_EW_CHARGE_GRAD 2
size_t mi_ewald_symmetry_scratch_bytes(void);
size_t mi_ewald_real_scratch_bytes(int n_atoms, int dtype);
int mi_ewald_real(const void* positions, const void* charges, const void* cell, const void* alpha /*[n_systems]*/,
                  const int32_t* batch_idx, int n_atoms, int dtype, const int32_t* idx_j,
                  const int32_t* unit_shifts, const int32_t* neighbor_ptr, int max_neighbors, int mask_value,
                  int flags, double* energies /*[n_atoms]*/, void* forces /*[n_atoms,3] dtype*/,
                  double* charge_grads /*[n_atoms]*/, void* scratch /*or NULL*/, size_t scratch_bytes, void* stream);
/* mi_ewald_real for a padded matrix that is KNOWN to be the unmodified output of a full (not half-filled) neighbour search: the caller passes
 * that search's num_neighbors array (counts that keep counting past the row width, as mi_nl_neighbors writes them).  A full list is symmetric
 * unless a row overflowed, so the per-entry checksums of the symmetry test are not computed (0.170 -> 0.138 ms on the 9 A headline list);
 * instead a row with search_num_neighbors[i] > max_neighbors raises the "not symmetric" mark, and every verify_stride-th row (0: none; rounded up to a power of two),
 * rotating with verify_phase, looks one of its entries (j, S) up in row j as (i, -S) and raises the mark when it is missing.  A marked call
 * takes the general scatter path of mi_ewald_real: results are those of the arrays as they ARE.  Rows are read up to their count only.
 * search_num_neighbors == NULL, a CSR list, or a scratch too small for checksums + records: exactly mi_ewald_real.  The Python host passes
 * the array only while matrix, shifts and counts carry the version counters the search left (neighborlist/_engine.py::FullListRecord).      */
int mi_ewald_real_listed(const void* positions, const void* charges, const void* cell, const void* alpha, const int32_t* batch_idx, int n_atoms,
                         int dtype, const int32_t* idx_j, const int32_t* unit_shifts, const int32_t* neighbor_ptr, int max_neighbors,
                         int mask_value, int flags, double* energies, void* forces, double* charge_grads, void* scratch, size_t scratch_bytes,
                         const int32_t* search_num_neighbors, int verify_stride, int verify_phase, void* stream);
/* mi_ewald_real_listed plus the virial of the listed entries, in the same owner pass: every stored entry e = (i -> j) contributes
 * fm_e r_a r_b (fm_e = 1/2 q_i q_j (erfc(a r)/r^3 + 2a/sqrt(pi) exp(-a^2 r^2)/r^2), r = r_j - r_i + S.cell), i.e. -dE/d(strain) of its energy
 * 1/2 q_i q_j erfc(a r)/r under x -> (I + eps) x with the unit shifts held fixed; per entry, so any list (full, half, asymmetric) is covered.
 * Each row's wave sums the six components {xx, yy, zz, xy, xz, yz} in fp64 and stores them in row_virial [n_atoms][6] (workspace, no
 * atomics); a fold pass writes virial_partial [n_systems][mi_ewald_virial_blocks()][6] (every entry, float64), the caller sums the block
 * dimension.  Energies, forces and charge gradients are those of mi_ewald_real_listed (same arithmetic).  n_systems > 1 needs batch_idx. */
int mi_ewald_real_virial(const void* positions, const void* charges, const void* cell, const void* alpha, const int32_t* batch_idx, int n_atoms,
                         int n_systems, int dtype, const int32_t* idx_j, const int32_t* unit_shifts, const int32_t* neighbor_ptr, int max_neighbors,
                         int mask_value, int flags, double* energies, void* forces, double* charge_grads, void* scratch, size_t scratch_bytes,
                         const int32_t* search_num_neighbors, int verify_stride, int verify_phase, double* row_virial, double* virial_partial,
                         void* stream);
int mi_ewald_virial_blocks(void);

/* Gaussian-smeared charges: the short-ranged pair correction that, added to a point-charge Ewald / PME / Coulomb energy, gives the energy of
 * Gaussian charge clouds of per-atom width sigma_i (sigma_i <= 0: point charge).  s = max(sigma, 0)^2, g_ij = sqrt(2 (s_i + s_j)), x = r / g_ij:
 *     energies[i] = -1/2 sum_{entries (i, j, S) of row i} q_i q_j erfc(x) / r,        r = r_j - r_i + S . cell
 * over a FULL (symmetric) list -- padded matrix (neighbor_ptr == NULL; entries equal to mask_value or outside [0, n_atoms) are padding) or CSR.
 * Entries with r <= 1e-8 or x >= 6 (erfc(6) = 2.2e-17) are skipped, and so are pairs of two point charges.  A half list is not detected.
 * The row owner writes every output (no atomics, deterministic).  Pair vector and r^2 in the positions dtype, everything else fp64 (libm erfc).
 * weights [n_atoms] float64 or NULL (all ones): entry weight w = (g_i + g_j) / 2 -- the outputs are then the derivatives of
 * L = sum_i g_i energies[i]:
 *   MI_GC_FORCES       forces [n_atoms][3] (positions dtype)  = -dL/dr_i = 2 sum_row w fm r,
 *                      fm = 1/2 q_i q_j (erfc(x)/r^3 + 2/(sqrt(pi) g_ij) exp(-x^2)/r^2)
 *   MI_GC_CHARGE_GRAD  charge_grads [n_atoms] float64         = dL/dq_i = -sum_row w q_j erfc(x)/r
 *   MI_GC_SIGMA_GRAD   sigma_grads [n_atoms] float64          = dL/dsigma_i = -(4/sqrt(pi)) q_i sigma_i sum_row w q_j exp(-x^2)/g_ij^3
 *   MI_GC_VIRIAL       system_partial[s][b][0..5] = block partials of -sum_entries w fm r_a r_b, {xx, yy, zz, xy, xz, yz}
 *   MI_GC_CELL_GRAD    system_partial[s][b][0..8] = block partials of dL/dcell[a][b] = sum_entries w fm S_a r_b (row-major; not with MI_GC_VIRIAL)
 * system_partial is [n_systems][mi_gaussian_charges_blocks()][mi_gaussian_charges_row_words()] float64; the caller sums the block dimension.
 * energies may be NULL (adjoint use).  cell NULL: non-periodic, unit_shifts must be NULL too.  unit_shifts NULL with a cell: all zero.
 * scratch: mi_gaussian_charges_scratch_bytes(n_atoms, dtype) bytes ({x, y, z, q, sigma} records + per-row tensors), contents undefined.
 * Self and neutralising-background terms are not part of this entry point (O(N), see nvalchemiops/interactions/electrostatics/gaussian.py). */
#define MI_GC_FORCES 1
#define MI_GC_CHARGE_GRAD 2
#define MI_GC_SIGMA_GRAD 4
#define MI_GC_VIRIAL 8
#define MI_GC_CELL_GRAD 16
size_t mi_gaussian_charges_scratch_bytes(int n_atoms, int dtype);
int mi_gaussian_charges_blocks(void);
int mi_gaussian_charges_row_words(void);
/* The per-system sums of the background term, in a fixed order (no atomics: bit-reproducible, unlike mi_segment_sum, whose one atomic per
 * wave leaves the last bit to the arrival order): partial [n_systems][mi_gaussian_charges_blocks()][3] float64 = block partials of
 * {sum q, sum q s, sum g q s} over each system's atoms, s = max(sigma, 0)^2, g = weights or 1 (NULL); the caller sums the block dimension. */
int mi_gaussian_charges_system_sums(const void* charges, const void* sigma, const double* weights, const int32_t* batch_idx, int n_atoms,
                                    int n_systems, int dtype, double* partial, void* stream);
int mi_gaussian_charges(const void* positions, const void* charges, const void* sigma, const void* cell /*[n_systems,3,3] or NULL*/,
                        const int32_t* batch_idx, const double* weights, int n_atoms, int n_systems, int dtype, const int32_t* idx_j,
                        const int32_t* unit_shifts, const int32_t* neighbor_ptr, int max_neighbors, int mask_value, int flags, double* energies,
                        void* forces, double* charge_grads, double* sigma_grads, double* system_partial, void* scratch, size_t scratch_bytes,
                        void* stream);

/* Point-dipole Ewald sum (csrc/dipole.hip; driver: nvalchemiops/interactions/electrostatics/dipole.py): what point dipoles mu_i (fixed in the
 * laboratory frame) add to the periodic energy of point charges q_i -- the charge-charge part is NOT included, the result is added to an Ewald /
 * PME energy.  Gaussian units, tin-foil boundary.  All arithmetic is fp64; only the pair vector and r^2 are formed in the positions dtype.  No
 * floating-point atomics, plain stores, fixed summation orders: every output is bit-reproducible.
 *
 * mi_ewald_dipole_real: over the stored entries (i, j, S) of a FULL (symmetric) list -- padded matrix (neighbor_ptr == NULL; entries equal to
 * mask_value or outside [0, n_atoms) are padding) or CSR -- with R = r_j - r_i + S . cell, r = |R|, a = alpha[system of i],
 *     B0 = erfc(a r)/r,  B_n = [(2n - 1) B_{n-1} + (2 a^2)^n / (a sqrt(pi)) exp(-a^2 r^2)] / r^2,  c_i = mu_i.R, c_j = mu_j.R, d = mu_i.mu_j,
 *     U = B1 (q_j c_i - q_i c_j + d) - B2 c_i c_j,        energies[i] = 1/2 sum_row U        (entries with r <= 1e-8 skipped, nothing else)
 * weights [n_atoms] float64 or NULL (all ones): entry weight w = (g_i + g_j) / 2 -- the outputs are then the derivatives of
 * L = sum_i g_i energies[i]:
 *   MI_DP_FORCES       forces [n_atoms][3] (positions dtype) = -dL/dr_i  = sum_row w dU/dR,
 *                      dU/dR = (-B2 (q_j c_i - q_i c_j + d) + B3 c_i c_j) R + (B1 q_j - B2 c_j) mu_i - (B1 q_i + B2 c_i) mu_j
 *   MI_DP_CHARGE_GRAD  charge_grads [n_atoms] float64        = dL/dq_i   = -sum_row w B1 c_j
 *   MI_DP_DIPOLE_GRAD  dipole_grads [n_atoms][3] float64     = dL/dmu_i  = sum_row w (B1 (q_j R + mu_j) - B2 c_j R)
 *   MI_DP_VIRIAL       virial_partial [n_systems][mi_ewald_dipole_blocks()][9] float64 = block partials of W[a][b] = -1/2 sum_entries w (dU/dR)_a R_b,
 *                      row-major and NOT symmetric (dU/dR is not along R); the caller sums the block dimension.  Needs unit_shifts.
 * energies may be NULL (adjoint use).  unit_shifts NULL: all zero.  A half list is not detected.  n_systems > 1 needs batch_idx.
 * scratch: mi_ewald_dipole_real_scratch_bytes(n_atoms, dtype) bytes ({x, y, z, q, mu} records + per-row virials), contents undefined.
 *
 * mi_ewald_dipole_structure_factors: table [n_systems][n_k][8] float64 = {Re S_q, Im S_q, Re M_x, Im M_x, Re M_y, Im M_y, Re M_z, Im M_z},
 * S_q = sum_j g_j q_j exp(i k.r_j), M = sum_j g_j mu_j exp(i k.r_j) over the atoms [system_ptr[s], system_ptr[s + 1]) of each system
 * (system_ptr NULL for one system), g = weights or 1 (NULL).  UNSCALED: the consumers apply G_k = (8 pi / V) exp(-k^2 / 4 a^2) / k^2
 * (half-space k set; k^2 < 1e-10: 0).  k_vectors [n_systems][n_k][3] in the positions dtype; every entry of the table is written.
 *
 * mi_ewald_dipole_recip_gather: with S = S_q + i k.M and A_i = (q_i - i k.mu_i) exp(-i k.r_i),
 *     energies[i] = 1/2 sum_k G_k { Re[A_i S] - q_i Re[exp(-i k.r_i) S_q] } - 2 a^3 / (3 sqrt(pi)) |mu_i|^2     (dipolar self term included)
 * and forces (positions dtype), charge_grads, dipole_grads [n_atoms][3] (float64) = -d/dr_i, d/dq_i, d/dmu_i of sum_i energies[i]; any output
 * may be NULL.  Adjoint form: table_g (the table summed with weights g) and weights together give the same derivatives of
 * L = sum_i g_i energies[i], i.e. 1/2 sum_k G_k Re[dA_i/dtheta (g_i S + S^g)] minus the charge part, and the self term times g_i.
 *
 * mi_ewald_dipole_recip_virial: virial [n_systems][9] float64, row-major, -dE/d(strain) of the reciprocal sum under x -> (I + eps) x with the
 * k set following the cell and the dipoles fixed (d(k.mu)/d eps_ab = -k_a mu_b):
 *     W[a][b] = sum_k e_k (delta_ab - 2 (1/k^2 + 1/(4 a^2)) k_a k_b) + G_k k_a (Im S Re M_b - Re S Im M_b),  e_k = 1/2 G_k (|S|^2 - |S_q|^2). */
#define MI_DP_FORCES 1
#define MI_DP_CHARGE_GRAD 2
#define MI_DP_DIPOLE_GRAD 4
#define MI_DP_VIRIAL 8
size_t mi_ewald_dipole_real_scratch_bytes(int n_atoms, int dtype);
int mi_ewald_dipole_blocks(void);
int mi_ewald_dipole_real(const void* positions, const void* charges, const void* dipoles, const void* cell /*[n_systems,3,3]*/,
                         const void* alpha /*[n_systems]*/, const int32_t* batch_idx, const double* weights, int n_atoms, int n_systems, int dtype,
                         const int32_t* idx_j, const int32_t* unit_shifts, const int32_t* neighbor_ptr, int max_neighbors, int mask_value, int flags,
                         double* energies, void* forces, double* charge_grads, double* dipole_grads, double* virial_partial, void* scratch,
                         size_t scratch_bytes, void* stream);
int mi_ewald_dipole_structure_factors(const void* positions, const void* charges, const void* dipoles, const double* weights, const void* k_vectors,
                                      const int32_t* system_ptr, int n_atoms, int n_systems, int n_k, int dtype, double* table, void* stream);
int mi_ewald_dipole_recip_gather(const void* positions, const void* charges, const void* dipoles, const void* k_vectors, const void* cell,
                                 const void* alpha, const int32_t* batch_idx, const double* table, const double* table_g, const double* weights,
                                 int n_atoms, int n_systems, int n_k, int dtype, double* energies, void* forces, double* charge_grads,
                                 double* dipole_grads, void* stream);
int mi_ewald_dipole_recip_virial(const double* table, const void* k_vectors, const void* cell, const void* alpha, int n_systems, int n_k, int dtype,
                                 double* virial, void* stream);

/* Point-quadrupole Ewald sum (csrc/quadrupole.hip; driver: nvalchemiops/interactions/electrostatics/quadrupole.py): what point quadrupoles Q_i
 * (symmetric Cartesian second Taylor coefficients 1/2 sum q d d, fixed in the laboratory frame; a traceless Stone quadrupole Theta is
 * Q = Theta / 3) add to the periodic energy of point charges q_i and point dipoles mu_i -- the charge-quadrupole, dipole-quadrupole and
 * quadrupole-quadrupole terms ONLY; the result is added to mi_ewald_dipole_* and an Ewald / PME energy.  quadrupoles is [n_atoms][3][3] in the
 * positions dtype; 1/2 (Q + Q^T) is used, tracelessness is not required.  Arithmetic, reproducibility, list formats, weights
 * (w = (g_i + g_j) / 2), scratch and virial layout are those of mi_ewald_dipole_*.
 *
 * mi_ewald_quadrupole_real: with B_n as for mi_ewald_dipole_real continued to B4 (B5 only for forces / virial), c = mu.R, t = tr Q, a = Q R,
 * s = R.a, m_ij = mu_i.a_j, m_ji = mu_j.a_i, p = a_i.a_j, d = Q_i:Q_j,
 *     C1 = -(q_i t_j + q_j t_i),  C2 = q_i s_j + q_j s_i + 2 (m_ji - m_ij) + t_i c_j - t_j c_i + t_i t_j + 2 d,
 *     C3 = c_i s_j - c_j s_i - t_i s_j - t_j s_i - 4 p,  C4 = s_i s_j,
 *     U = B1 C1 + B2 C2 + B3 C3 + B4 C4,        energies[i] = 1/2 sum_row U        (entries with r <= 1e-8 skipped, nothing else)
 *   MI_QD_FORCES          forces [n_atoms][3] (positions dtype) = -dL/dr_i = sum_row w dU/dR (csrc/quadrupole.hip states dU/dR)
 *   MI_QD_CHARGE_GRAD     charge_grads [n_atoms] float64       = dL/dq_i  = sum_row w (B2 s_j - B1 t_j)
 *   MI_QD_DIPOLE_GRAD     dipole_grads [n_atoms][3] float64    = dL/dmu_i = sum_row w ((B3 s_j - B2 t_j) R - 2 B2 a_j)   (independent of every mu)
 *   MI_QD_QUADRUPOLE_GRAD quadrupole_grads [n_atoms][3][3] float64, symmetric = dL/dQ_i
 *                         = sum_row w (A0 I + A1 R R^T + B2 (mu_j R^T + R mu_j^T) - 2 B3 (R a_j^T + a_j R^T) + 2 B2 Q_j),
 *                         A0 = -B1 q_j + B2 (c_j + t_j) - B3 s_j,  A1 = B2 q_j - B3 (c_j + t_j) + B4 s_j
 *   MI_QD_VIRIAL          virial_partial [n_systems][mi_ewald_quadrupole_blocks()][9] float64, W[a][b] = -1/2 sum_entries w (dU/dR)_a R_b, row-major
 *                         and NOT symmetric; the caller sums the block dimension.  Needs unit_shifts.
 * scratch: mi_ewald_quadrupole_real_scratch_bytes(n_atoms, dtype) bytes (16-word records {x, y, z, q, mu, Q(6), -} + per-row virials).
 *
 * mi_ewald_quadrupole_structure_factors: table [n_systems][n_k][10] float64 = {Re, Im} of {S_q, M_x, M_y, M_z, T}, T = sum_j g_j (k.Q_j.k)
 * exp(i k.r_j), S_q and M as for the dipole table; table_v [n_systems][n_k][6] = {Re, Im} of V = sum_j g_j (Q_j k) exp(i k.r_j), or NULL
 * (only the virial reads it).  UNSCALED.
 *
 * mi_ewald_quadrupole_recip_gather: with S' = S_q + i k.M, tau_i = k.Q_i.k, e_i = exp(i k.r_i),
 *     energies[i] = 1/2 sum_k G_k { tau_i Re[conj(e_i) (T - S')] - Re[conj((q_i + i k.mu_i) e_i) T] }
 *                   + 4 a^3 / (3 sqrt(pi)) q_i tr Q_i - 4 a^5 / (5 sqrt(pi)) (2 Q_i:Q_i + (tr Q_i)^2)                  (self term included)
 * and forces, charge_grads, dipole_grads, quadrupole_grads [n_atoms][3][3] as above; any output may be NULL; adjoint form as for
 * mi_ewald_dipole_recip_gather.
 *
 * mi_ewald_quadrupole_recip_virial: virial [n_systems][9] float64, row-major, with d(k.mu)/d eps_ab = -k_a mu_b, d(k.Q.k)/d eps_ab = -2 k_a (Q k)_b:
 *     W[a][b] = sum_k e_k (delta_ab - 2 (1/k^2 + 1/(4 a^2)) k_a k_b) + G_k k_a (2 Re[conj(T - S') V_b] - (Im T Re M_b - Re T Im M_b)),
 *     e_k = 1/2 G_k (|T|^2 - 2 Re[conj(S') T]). */
#define MI_QD_FORCES 1
#define MI_QD_CHARGE_GRAD 2
#define MI_QD_DIPOLE_GRAD 4
#define MI_QD_VIRIAL 8
#define MI_QD_QUADRUPOLE_GRAD 16
size_t mi_ewald_quadrupole_real_scratch_bytes(int n_atoms, int dtype);
int mi_ewald_quadrupole_blocks(void);
int mi_ewald_quadrupole_real(const void* positions, const void* charges, const void* dipoles, const void* quadrupoles,
                             const void* cell /*[n_systems,3,3]*/, const void* alpha /*[n_systems]*/, const int32_t* batch_idx,
                             const double* weights, int n_atoms, int n_systems, int dtype, const int32_t* idx_j, const int32_t* unit_shifts,
                             const int32_t* neighbor_ptr, int max_neighbors, int mask_value, int flags, double* energies, void* forces,
                             double* charge_grads, double* dipole_grads, double* quadrupole_grads, double* virial_partial, void* scratch,
                             size_t scratch_bytes, void* stream);
int mi_ewald_quadrupole_structure_factors(const void* positions, const void* charges, const void* dipoles, const void* quadrupoles,
                                          const double* weights, const void* k_vectors, const int32_t* system_ptr, int n_atoms, int n_systems,
                                          int n_k, int dtype, double* table, double* table_v, void* stream);
int mi_ewald_quadrupole_recip_gather(const void* positions, const void* charges, const void* dipoles, const void* quadrupoles,
                                     const void* k_vectors, const void* cell, const void* alpha, const int32_t* batch_idx, const double* table,
                                     const double* table_g, const double* weights, int n_atoms, int n_systems, int n_k, int dtype,
                                     double* energies, void* forces, double* charge_grads, double* dipole_grads, double* quadrupole_grads,
                                     void* stream);
int mi_ewald_quadrupole_recip_virial(const double* table, const double* table_v, const void* k_vectors, const void* cell, const void* alpha,
                                     int n_systems, int n_k, int dtype, double* virial, void* stream);

/* Thole damping of point dipoles, exponential form (the AMOEBA smearing; csrc/dipole.hip, the second radial kind of the pair kernel of
 * mi_ewald_dipole_real; driver: nvalchemiops/interactions/electrostatics/thole.py): the short-ranged real-space correction that, ADDED to the
 * energy of undamped point dipoles (mi_ewald_dipole_*, mi_pme_dipole_*), smears the charge-dipole and dipole-dipole terms.  Charge-charge terms
 * are not touched, and nothing depends on an Ewald alpha.  Over the stored entries (i, j, S) of a FULL list, R = r_j - r_i + S . cell, r = |R|,
 * a = polarizability [n_atoms] (positions dtype), E = thole_a r^3 / sqrt(a_i a_j):
 *     D1 = -e^-E / r^3,  D2 = -3 (1 + E) e^-E / r^5,  D3 = -15 (1 + E + 3/5 E^2) e^-E / r^7
 *     U = D1 (q_j c_i - q_i c_j + d) - D2 c_i c_j,        energies[i] = 1/2 sum_row U
 * i.e. mi_ewald_dipole_real's expressions with D_n in place of B_n; arguments, weights (w = (g_i + g_j) / 2), flags, outputs, virial layout,
 * arithmetic model (pair vector and r^2 in the positions dtype, the rest fp64, libm exp) and bit-reproducibility are those of
 * mi_ewald_dipole_real.  An entry contributes exactly 0 when either end has a <= 0 or NaN (not polarisable: not damped), when r <= 1e-8, and
 * when E >= 50 (it leaves before the exp; (1 + E + 0.6 E^2) e^-E < 4e-19 there).  Self-image entries (i, i, S != 0) are kept.
 *   MI_DP_POLAR_GRAD   polarizability_grads [n_atoms] float64 = dL/da_i = -1 / (2 a_i) sum_row w E X,
 *                      X = dU/dE at fixed R = (e^-E / r^3)(q_j c_i - q_i c_j + d) - (3 E e^-E / r^5) c_i c_j     (0 for a_i <= 0)
 * cell may be NULL (a cluster: unit_shifts must be NULL too, no virial).  thole_a must be positive and finite.
 * scratch: mi_thole_dipole_scratch_bytes(n_atoms, dtype) bytes ({x, y, z, q, mu, a} records + per-row virials), contents undefined.
 * virial_partial is [n_systems][mi_thole_dipole_blocks()][9]. */
#define MI_DP_POLAR_GRAD 16
size_t mi_thole_dipole_scratch_bytes(int n_atoms, int dtype);
int mi_thole_dipole_blocks(void);
int mi_thole_dipole(const void* positions, const void* charges, const void* dipoles, const void* cell /*[n_systems,3,3] or NULL*/,
                    const void* polarizability /*[n_atoms]*/, double thole_a, const int32_t* batch_idx, const double* weights, int n_atoms,
                    int n_systems, int dtype, const int32_t* idx_j, const int32_t* unit_shifts, const int32_t* neighbor_ptr, int max_neighbors,
                    int mask_value, int flags, double* energies, void* forces, double* charge_grads, double* dipole_grads,
                    double* polarizability_grads, double* virial_partial, void* scratch, size_t scratch_bytes, void* stream);

/* Cluster point multipoles: the bare (undamped, 1/r) multipole pair sums (csrc/dipole.hip and csrc/quadrupole.hip, one more radial kind of the
 * pair kernels of mi_ewald_dipole_real / mi_ewald_quadrupole_real; driver: nvalchemiops/interactions/electrostatics/cluster.py).  The radial
 * factors are the alpha -> 0 limit of the Ewald B_n:
 *     B1 = 1 / r^3,  B_{n+1} = (2n + 1) B_n / r^2:  B2 = 3 / r^5,  B3 = 15 / r^7,  B4 = 105 / r^9,  B5 = 945 / r^11
 * with no erfc and no exp.  Everything else -- the pair expressions U, dU/dR, dU/dq, dU/dmu, dU/dQ, arguments, weights (w = (g_i + g_j) / 2),
 * flags (MI_DP_* / MI_QD_*), outputs, virial layout, list formats, padding, the r <= 1e-8 skip, kept self-image entries, the arithmetic model
 * (pair vector and r^2 in the positions dtype, the rest fp64) and bit-reproducibility -- is that of mi_ewald_dipole_real and
 * mi_ewald_quadrupole_real, without their alpha argument.
 * mi_coulomb_dipole: the charge-dipole and dipole-dipole energy over the stored entries of a FULL list; added to a bare charge-charge sum.
 * mi_coulomb_quadrupole: the terms with at least one quadrupole; added to mi_coulomb_dipole.
 * cell may be NULL (a cluster: unit_shifts must be NULL too, no virial); with a cell and unit_shifts the sum runs over the listed images (a
 * cut-off sum: the list is the cutoff).  An unknown flag bit is an argument error.
 * scratch: mi_coulomb_dipole_scratch_bytes / mi_coulomb_quadrupole_scratch_bytes(n_atoms, dtype) bytes (records + per-row virials), contents
 * undefined.  virial_partial is [n_systems][mi_coulomb_dipole_blocks() / mi_coulomb_quadrupole_blocks()][9]. */
size_t mi_coulomb_dipole_scratch_bytes(int n_atoms, int dtype);
int mi_coulomb_dipole_blocks(void);
int mi_coulomb_dipole(const void* positions, const void* charges, const void* dipoles, const void* cell /*[n_systems,3,3] or NULL*/,
                      const int32_t* batch_idx, const double* weights, int n_atoms, int n_systems, int dtype, const int32_t* idx_j,
                      const int32_t* unit_shifts, const int32_t* neighbor_ptr, int max_neighbors, int mask_value, int flags, double* energies,
                      void* forces, double* charge_grads, double* dipole_grads, double* virial_partial, void* scratch, size_t scratch_bytes,
                      void* stream);
size_t mi_coulomb_quadrupole_scratch_bytes(int n_atoms, int dtype);
int mi_coulomb_quadrupole_blocks(void);
int mi_coulomb_quadrupole(const void* positions, const void* charges, const void* dipoles, const void* quadrupoles,
                          const void* cell /*[n_systems,3,3] or NULL*/, const int32_t* batch_idx, const double* weights, int n_atoms,
                          int n_systems, int dtype, const int32_t* idx_j, const int32_t* unit_shifts, const int32_t* neighbor_ptr,
                          int max_neighbors, int mask_value, int flags, double* energies, void* forces, double* charge_grads,
                          double* dipole_grads, double* quadrupole_grads, double* virial_partial, void* scratch, size_t scratch_bytes,
                          void* stream);

/* Scaled bonded pairs of point multipoles (csrc/pair_scale.hip; driver: nvalchemiops/interactions/electrostatics/pair_scale.py).  Every
 * stored entry e = (i, j, S) of a FULL list carries a scale pair_scales[e] (float64, laid out like idx_j: [n_atoms][max_neighbors] or
 * [nnz]; symmetric, s_ij = s_ji, which is not checked).  Returned is what has to be ADDED to an unscaled total so that every listed pair
 * carries its scale:
 *     E_i = 1/2 sum_{row i} (s_e - 1) U_ij,   U_ij = L_i L_j (1 / r)
 * the complete bare pair energy of charges, dipoles and quadrupoles: the charge-charge term B0 q_i q_j plus the pair expressions of
 * mi_coulomb_dipole and mi_coulomb_quadrupole (B0 = 1 / r, B1 = 1 / r^3, B_{n+1} = (2n + 1) B_n / r^2), with their gradients.  s_e = 0 is an
 * exclusion; an entry with s_e = 1 is skipped before any arithmetic and contributes exactly 0.  dipoles and quadrupoles may be NULL (none).
 * One group of 8 lanes per row (8 rows per wave64), butterfly sums inside the group, no atomics: bit-reproducible.
 * Arguments, weights (an entry weighs (g_i + g_j) / 2 . (s_e - 1)), flags (MI_QD_*), outputs, virial layout, list formats, padding (the scale
 * of a padding slot is not looked at), the r <= 1e-8 skip and the arithmetic model are those of mi_coulomb_quadrupole.  minimum_image != 0
 * (needs a cell, excludes unit_shifts): the difference r_j - r_i of every entry is reduced to its minimum image in fp64 (rint of the
 * fractional components) and rounded once to the positions dtype; the virial then uses the reduced vector.  An unknown flag bit,
 * minimum_image without a cell and unit_shifts together with minimum_image are argument errors; the virial needs unit_shifts or
 * minimum_image.
 * scratch: mi_pair_scale_scratch_bytes(n_atoms, dtype) bytes (records + per-row virials), contents undefined.  virial_partial is
 * [n_systems][mi_pair_scale_blocks()][9]. */
size_t mi_pair_scale_scratch_bytes(int n_atoms, int dtype);
int mi_pair_scale_blocks(void);
int mi_pair_scale(const void* positions, const void* charges, const void* dipoles /*or NULL*/, const void* quadrupoles /*or NULL*/,
                  const void* cell /*[n_systems,3,3] or NULL*/, const int32_t* batch_idx, const double* weights, const double* pair_scales,
                  int n_atoms, int n_systems, int dtype, const int32_t* idx_j, const int32_t* unit_shifts, const int32_t* neighbor_ptr,
                  int max_neighbors, int mask_value, int minimum_image, int flags, double* energies, void* forces, double* charge_grads,
                  double* dipole_grads, double* quadrupole_grads, double* virial_partial, void* scratch, size_t scratch_bytes, void* stream);

/* Charge equilibration (csrc/qeq.hip; driver: nvalchemiops/interactions/electrostatics/qeq.py): the real-space Hessian of the Gaussian-charge
 * electrostatic energy as a stored sparse operator over the caller's FULL list, its product, and the vector kernels of a batched projected
 * conjugate-gradient solve of  min_q sum chi_i q_i + 1/2 sum J_i q_i^2 + E_el(q),  sum_{i in s} q_i = Q_s.  All arithmetic is fp64; only the
 * pair vector and r are formed in the positions dtype.  No atomics anywhere: every per-system sum is a fixed-order fold into
 * mi_qeq_blocks() block partials that the next kernel sums itself, so these entry points are bit-reproducible (a periodic solve also calls the
 * reciprocal-space entry points, which are not).  Nothing synchronises with the host.  n_systems <= 65535 wherever per-system sums are formed
 * (one grid row per system; every block scans batch_idx: O(n_atoms n_systems) index reads per launch).
 *
 * mi_qeq_pair_coefficients (once per geometry): for every slot e of the list layout -- padded matrix [n_atoms][max_neighbors]
 *   (neighbor_ptr == NULL) or CSR -- with row i, neighbour j, unit shift S, r = |r_j - r_i + S . cell|, g_ij = sqrt(2 (s_i + s_j)), s = max(sigma, 0)^2:
 *     coefficients[e] = [erfc_AS(alpha_s r) - erfc(r / g_ij)] / r   with a cell (erfc_AS: the polynomial of mi_ewald_real; erfc: libm, as mi_gaussian_charges)
 *     coefficients[e] = [1 - erfc(r / g_ij)] / r                    cell == NULL (alpha is not read; unit_shifts must be NULL)
 *     neighbors[e]    = j
 *   r <= 1e-8: no contribution.  The erfc(r / g_ij) term is dropped for r / g_ij >= 6 and for two point charges, as mi_gaussian_charges does.
 *   Padding (matrix entries equal to mask_value, any index outside [0, n_atoms)) and entries without contribution get coefficient 0 and
 *   neighbors[e] = i, so neighbors[] is always safe to gather with.  12 bytes per slot.
 *     diagonal[i]     = hardness[i] + [sigma_i > 0] / (sqrt(pi) sigma_i)
 *   sigma, cell [n_systems,3,3], alpha [n_systems] in the positions dtype; hardness float64.  batch_idx is read only with a cell and n_systems > 1.
 * mi_qeq_apply:  y[i] = (y_in ? y_in[i] : 0) + diagonal[i] x[i] + sum_{slots e of row i} coefficients[e] x[neighbors[e]]   (one wave64 per row;
 *   y_in may be y, x must not be).  partial (may be NULL): [n_systems][mi_qeq_blocks()][2] block partials of {sum_i y_i, sum_i x_i y_i} per system.
 * State of a solve: [n_systems][mi_qeq_state_words()] float64 = {r.r, b.b, done, iterations, alpha, beta, -, -}; every kernel reads state_in
 *   and writes state_out (two buffers used alternately; a fresh solve starts from zeros).  counts [n_systems] float64 = atoms per system.
 * mi_qeq_cg_update(mode 0): from partial_y = the partials of y = H p:  w = y - mean_s(y),  alpha_s = r.r / p.y,  q += alpha p,  r -= alpha w,
 *   partial_rr [n_systems][mi_qeq_blocks()] = block partials of the new r.r.  A done system, or one with p.y <= 0 (then marked done), is not touched.
 *   mode 1 (set-up): r = -(y - mean_s(y)) for y = chi + H q0; q and p are not used.
 * mi_qeq_cg_direction(mode 0): beta_s = r.r_new / r.r_old,  p = r + beta p,  iterations += 1,  done = r.r_new <= tolerance^2 b.b; done systems
 *   are frozen.  mode 1 (set-up): b.b = r.r, p = r, iterations = 0, done at once when b.b == 0 (also one-atom and empty systems).
 *   mode 2 (restart, warm start): as mode 1 but b.b is kept from state_in. */
int mi_qeq_blocks(void);
int mi_qeq_state_words(void);
int mi_qeq_pair_coefficients(const void* positions, const void* sigma, const double* hardness, const void* cell /*[n_systems,3,3] or NULL*/,
                             const void* alpha /*[n_systems], NULL without a cell*/, const int32_t* batch_idx, int n_atoms, int n_systems, int dtype,
                             const int32_t* idx_j, const int32_t* unit_shifts, const int32_t* neighbor_ptr, int max_neighbors, int mask_value,
                             double* coefficients, int32_t* neighbors, double* diagonal, void* stream);
int mi_qeq_apply(const double* coefficients, const int32_t* neighbors, const double* diagonal, const double* x, const double* y_in,
                 const int32_t* batch_idx, int n_atoms, int n_systems, const int32_t* neighbor_ptr, int max_neighbors, double* y, double* partial,
                 void* stream);
int mi_qeq_cg_update(const double* y, const double* partial_y, const double* counts, const int32_t* batch_idx, int n_atoms, int n_systems, int mode,
                     double* q, double* r, const double* p, const double* state_in, double* state_out, double* partial_rr, void* stream);
int mi_qeq_cg_direction(const double* partial_rr, const int32_t* batch_idx, int n_atoms, int n_systems, int mode, double tolerance, const double* r,
                        double* p, const double* state_in, double* state_out, void* stream);

/* Induced point dipoles (csrc/induced.hip; driver: nvalchemiops/interactions/electrostatics/induced.py): the real-space dipole-dipole operator
 * of the point-dipole Ewald sum as a stored sparse operator of 3 x 3 blocks over the caller's FULL list, its product, and the vector kernels of
 * a batched Jacobi-preconditioned conjugate-gradient solve of  H mu = b,  H = diag(1 / a) + T.  All arithmetic is fp64; only the pair vector
 * and r are formed in the positions dtype.  No atomics anywhere: every per-system sum is a fixed-order fold into mi_induced_blocks() block
 * partials that the next kernel sums itself, so these entry points are bit-reproducible.  Nothing synchronises with the host.
 * n_systems <= 65535 wherever per-system sums are formed (one grid row per system; every block scans batch_idx).
 * Solver vectors (x, y, y_in, r, p) are dense [n_atoms][3] float64.
 *
 * mi_induced_pair_tensors (once per geometry): for every slot e of the list layout -- padded matrix [n_atoms][max_neighbors]
 *   (neighbor_ptr == NULL, n_slots = n_atoms * max_neighbors) or CSR (n_slots entries) -- with row i, neighbour j, unit shift S,
 *   R = r_j - r_i + S . cell, r = |R|, formed as mi_ewald_dipole_real forms them (libm erfc / exp):
 *     tensors[0][e] = B1, tensors[1][e] = B2, tensors[2..5)[e] = R      (five streams of n_slots float64: T_e = B1 I - B2 R R^T)
 *     neighbors[e]  = j                                                  44 bytes per slot
 *   r <= 1e-8: no contribution.  Padding (matrix entries equal to mask_value, any index outside [0, n_atoms)), entries without contribution
 *   and entries with a non-polarisable atom at either end get zero coefficients and neighbors[e] = i, so neighbors[] is always safe to gather
 *   with.  diagonal[i] = 1 / a_i, preconditioner[i] = a_i; an atom with a_i <= 0 or NaN is not polarisable: both are 1 and its row is empty.
 *   polarizability, cell [n_systems,3,3], alpha [n_systems] in the positions dtype.  unit_shifts may be NULL (no translations).
 * mi_thole_induced_pair_tensors: the same with exponential Thole damping of width thole_a (> 0, finite): tensors[0][e] = B1 + D1,
 *   tensors[1][e] = B2 + D2 with the D_n and the E >= 50 exit of mi_thole_dipole, same streams and layout, so mi_induced_apply then gives
 *   diagonal x + dE/dmu of mi_ewald_dipole_real + mi_thole_dipole at zero charges.  Everything else in this section is used unchanged.
 * mi_cluster_induced_pair_tensors: the operator of a cluster without a cell -- no cell, no alpha, no shifts, no batch_idx (the list confines
 *   pairs to systems): tensors[0][e] = 1 / r^3, tensors[1][e] = 3 / r^5 (the alpha -> 0 limit of B1, B2) for thole_a == 0, and those plus
 *   D1, D2 of mi_thole_dipole (with its E >= 50 exit) for a finite thole_a > 0; any other thole_a is an argument error.  Same streams, layout,
 *   padding and non-polarisable rules, so mi_induced_apply then gives diagonal x + dE/dmu of mi_coulomb_dipole (+ mi_thole_dipole) at zero
 *   charges, and the product and CG entry points of this section are used unchanged.
 * mi_induced_apply:  y[i] = (y_in ? y_in[i] : 0) + diagonal[i] x[i] + sum_{slots e of row i} (B1 x[j] - B2 (R . x[j]) R)   (one wave64 per row,
 *   mi_induced_unroll_depth() trips in flight; y_in is added as given; x, y_in and y must not overlap).
 *   partial (may be NULL): [n_systems][mi_induced_blocks()] block partials of sum_i x_i . y_i per system.  mi_induced_dot: those partials alone.
 * State of a solve: [n_systems][mi_induced_state_words()] float64 = {r.z, b.b, done, iterations, alpha, beta, breakdown, r.r}; every kernel
 *   reads state_in and writes state_out (two buffers used alternately; a fresh solve starts from zeros).
 * mi_induced_cg_update(mode 0): from partial_y = the partials of y = H p:  alpha_s = r.z / p.y,  x += alpha p,  r -= alpha y,
 *   partial_rr [n_systems][mi_induced_blocks()][2] = block partials of the new {r.r, r.z}, z = preconditioner * r.  A done system is not
 *   touched.  A system that is not done and has p.y <= 0 or not finite is frozen (done = 1) with breakdown = 1: the operator is not positive
 *   definite.  mode 1 (set-up): r = -y for y = H x0 - b; x, p and partial_y are not used.
 * mi_induced_cg_direction(mode 0): beta_s = r.z_new / r.z_old,  p = z + beta p,  iterations += 1,  done = r.r_new <= tolerance^2 b.b; done
 *   systems are frozen.  mode 1 (set-up): b.b = r.r, p = z, iterations = 0, done at once when b.b == 0.  mode 2 (restart): as mode 1 but b.b
 *   is kept from state_in. */
int mi_induced_blocks(void);
int mi_induced_state_words(void);
int mi_induced_tensor_words(void);
int mi_induced_unroll_depth(void);
int mi_induced_pair_tensors(const void* positions, const void* polarizability, const void* cell /*[n_systems,3,3]*/, const void* alpha /*[n_systems]*/,
                            const int32_t* batch_idx, int n_atoms, int n_systems, int dtype, const int32_t* idx_j, const int32_t* unit_shifts,
                            const int32_t* neighbor_ptr, int max_neighbors, int mask_value, long long n_slots, double* tensors, int32_t* neighbors,
                            double* diagonal, double* preconditioner, void* stream);
int mi_thole_induced_pair_tensors(const void* positions, const void* polarizability, const void* cell /*[n_systems,3,3]*/,
                                  const void* alpha /*[n_systems]*/, const int32_t* batch_idx, int n_atoms, int n_systems, int dtype,
                                  const int32_t* idx_j, const int32_t* unit_shifts, const int32_t* neighbor_ptr, int max_neighbors, int mask_value,
                                  long long n_slots, double* tensors, int32_t* neighbors, double* diagonal, double* preconditioner,
                                  double thole_a, void* stream);
int mi_cluster_induced_pair_tensors(const void* positions, const void* polarizability, int n_atoms, int dtype, const int32_t* idx_j,
                                    const int32_t* neighbor_ptr, int max_neighbors, int mask_value, long long n_slots, double* tensors,
                                    int32_t* neighbors, double* diagonal, double* preconditioner, double thole_a, void* stream);
int mi_induced_apply(const double* tensors, const int32_t* neighbors, const double* diagonal, const double* x, const double* y_in,
                     const int32_t* batch_idx, int n_atoms, int n_systems, const int32_t* neighbor_ptr, int max_neighbors, long long n_slots,
                     double* y, double* partial, void* stream);
int mi_induced_dot(const double* x, const double* y, const int32_t* batch_idx, int n_atoms, int n_systems, double* partial, void* stream);
int mi_induced_cg_update(const double* y, const double* partial_y, const double* preconditioner, const int32_t* batch_idx, int n_atoms,
                         int n_systems, int mode, double* x, double* r, const double* p, const double* state_in,
                         double* state_out, double* partial_rr, void* stream);
int mi_induced_cg_direction(const double* partial_rr, const double* preconditioner, const int32_t* batch_idx, int n_atoms, int n_systems,
                            int mode, double tolerance, const double* r, double* p, const double* state_in, double* state_out,
                            void* stream);

/* Explicit-k reciprocal-space Ewald.  Replaces `alchemiops::_[batch_]ewald_reciprocal_space_energy[_forces
 * [_charge_grad]]` (ewald.py:1365-2318; kernels ewald_kernels.py:1496-2480).  Two passes, no [K,N] phase tables:
 *   mi_ewald_structure_factors : S[b][k] = 8pi/V exp(-k^2/4a^2)/k^2 * sum_j w_j exp(i k.r_j) (interleaved re,im; k^2<1e-10 -> 0)
 *                                total_charge[b] = sum_j w_j / V (0 when n_k < 2, as the reference's k_idx==1 accumulation)
 *   mi_ewald_recip_gather      : phi_i = sum_k Re(S_k exp(-i k.r_i)), kforce_i = sum_k (S_re sin - S_im cos) k, and from them
 *                                E_i = q phi/2 - a q^2/sqrt(pi) - pi q Q/(2a^2), F_i = q kforce_i, dE/dq_i = phi - 2a q/sqrt(pi) - pi Q/a^2
 * k_vectors [n_systems,n_k,3] in `dtype` (half-space set); system_ptr [n_systems+1] atom ranges (NULL: one system);
 * total_charge NULL in the gather = no self/background corrections (used by the adjoint).  Any output pointer may be NULL.  */
/* Virial of the explicit-k reciprocal sum from mi_ewald_structure_factors' output (S_k = G_k sum_j q_j exp(i k.r_j)): E_k = |S_k|^2 / (2 G_k),
 * W[a][b] = sum_k E_k (delta_ab - 2 (1/k^2 + 1/(4 alpha^2)) k_a k_b) over the caller's half-space set (k_vectors [n_systems,n_k,3] in `dtype`,
 * reciprocal vectors of `cell`).  partial [n_systems][mi_ewald_recip_virial_blocks()][6] float64 {xx, yy, zz, xy, xz, yz}, every entry
 * written; the caller folds the blocks and adds the background term.                                                                          */
int mi_ewald_recip_virial(const double* structure_factors, const void* k_vectors, const void* cell, const void* alpha, int n_systems, int n_k,
                          int dtype, double* partial, void* stream);
int mi_ewald_recip_virial_blocks(void);
int mi_ewald_structure_factors(const void* positions, const void* weights /*[n_atoms] dtype*/, const void* k_vectors, const void* cell,
                               const void* alpha, const int32_t* system_ptr, int n_atoms, int n_systems, int n_k,
                               int max_atoms_per_system, int dtype, double* structure_factors /*[n_systems,n_k,2]*/,
                               double* total_charge /*[n_systems]*/, void* stream);
int mi_ewald_recip_gather(const void* positions, const void* charges, const void* k_vectors, const void* alpha, const int32_t* batch_idx,
                          const double* structure_factors, const double* total_charge, int n_atoms, int n_k, int dtype,
                          double* potential /*[n_atoms]*/, double* kforce /*[n_atoms,3]*/, double* energies /*[n_atoms]*/,
                          void* forces /*[n_atoms,3] dtype*/, double* charge_grads /*[n_atoms]*/, void* stream);

/* out[i] = sum_k k (weights[i] . k) (S_re cos + S_im sin)(k.r_i), float64 [n_atoms,3]: position derivative of sum_i weights_i . kforce_i at
 * fixed structure factors; one term of the adjoint of the explicit-k FORCES ("forces" is in the grad_arrays of
 * alchemiops::_[batch_]ewald_reciprocal_space_energy_forces*, ewald.py:1486-1496; the reference replays its tape).                       */
int mi_ewald_recip_gather_kk(const void* positions, const void* k_vectors, const int32_t* batch_idx, const double* structure_factors,
                             const double* weights /*[n_atoms,3]*/, int n_atoms, int n_k, int dtype, double* out /*[n_atoms,3]*/, void* stream);

/* Adjoint of mi_ewald_real w.r.t. positions / charges / cell / alpha for L = sum_i g_i E_i (replaces the Warp-tape backward of
 * the real-space ops, autograd.py:525-665 + the generated adjoints of ewald_kernels.py:266-1495).  Owner-only like the forward:
 *   dL/dr_i = sum_j (g_i+g_j) fm_ij sep_ij ; dL/dq_i = sum_j 1/2 (g_i+g_j) q_j erfc(a r)/r ;
 *   dL/dcell[s][a][b] = -sum_i g_i sum_j fm_ij sep_ij[b] S_ij[a] ; dL/dalpha[s] = -sum_i g_i sum_j q_i q_j exp(-a^2 r^2)/sqrt(pi).
 * grad_cell / grad_alpha ([n_systems,3,3] / [n_systems], float64, zeroed by the caller) may be NULL.  `symmetry_scratch` as in
 * mi_ewald_real: a list that is not symmetric gets the general adjoint (entry (i -> j) carries g_i to both ends, atomics).      */
size_t mi_ewald_real_bwd_scratch_bytes(int n_systems); /* symmetry checksums + slotted partials of the per-system sums (grad_cell / grad_alpha) */
int mi_ewald_real_bwd(const void* positions, const void* charges, const void* cell, const void* alpha, const int32_t* batch_idx,
                      int n_atoms, int n_systems, int dtype, const int32_t* idx_j, const int32_t* unit_shifts, const int32_t* neighbor_ptr,
                      int max_neighbors, int mask_value, const void* grad_energies /*[n_atoms] dtype*/,
                      void* grad_positions /*[n_atoms,3] dtype*/, void* grad_charges /*[n_atoms] dtype*/,
                      double* grad_cell, double* grad_alpha, void* symmetry_scratch /*or NULL*/,
                      size_t scratch_bytes /* >= mi_ewald_symmetry_scratch_bytes(); with mi_ewald_real_bwd_scratch_bytes(n_systems) the per-system
                                              sums go through 64 slots per system instead of one atomic address */,
                      void* stream);

/* Adjoint of the explicit FORCES and CHARGE GRADIENTS of mi_ewald_real for L = sum_k w_k . F_k + sum_k v_k cg_k (second derivatives of the
 * pair sum; the reference differentiates these outputs through the Warp tape: "forces" and "charge_gradients" are in the grad_arrays of the
 * `_energy_forces*` ops, ewald.py:343-348, :606-612).  grad_forces / grad_charge_grads: either may be NULL.  Entry-wise scatter, valid for
 * any list; with `scratch` (mi_ewald_real_bwd_scratch_bytes(n_systems)) the list is checksummed in an owner-only pass first (no atomics: the
 * mirrored entry of a symmetric list contributes the same amount) and the scatter pass only runs when the list is NOT symmetric.  All gradient outputs are float64 and zeroed by the library; grad_cell / grad_alpha may be NULL.                                */
int mi_ewald_real_forces_bwd(const void* positions, const void* charges, const void* cell, const void* alpha, const int32_t* batch_idx,
                             int n_atoms, int n_systems, int dtype, const int32_t* idx_j, const int32_t* unit_shifts,
                             const int32_t* neighbor_ptr, int max_neighbors, int mask_value, const void* grad_forces /*[n_atoms,3] dtype or NULL*/,
                             const void* grad_charge_grads /*[n_atoms] dtype or NULL*/, double* grad_positions /*[n_atoms,3]*/,
                             double* grad_charges /*[n_atoms]*/, double* grad_cell /*[n_systems,3,3]*/, double* grad_alpha /*[n_systems]*/,
                             void* scratch /*or NULL; mi_ewald_real_bwd_scratch_bytes(n_systems): slotted per-system sums*/, size_t scratch_bytes, void* stream);

/* ---- cut-off Coulomb ---------------------------------------------------------------------------
 * Replaces the eight alchemiops::_[batch_]coulomb_energy[_forces]_{list,matrix} ops (interactions/electrostatics/coulomb.py:716-1330;
 * kernels :133-708).  float64 only, as the reference upcasts before the launch (:1423-1426).  Pair term over each stored entry
 * (i, j): r_ij = r_i - r_j - cell^T S, skipped when r >= cutoff or r < 1e-10; phi = erfc_AS(alpha r)/r for alpha > 0, else 1/r.
 *   energies[i] = energy_prefactor * sum_j q_i q_j phi          (plain store; the reference atomically adds into zeros)
 *   forces      : += f_ij on i and -= f_ij on j with f_ij = 1/2 q_i q_j (-phi'(r)/r) r_ij -- the reference's scatter, valid for
 *                 full, half and asymmetric lists (fp64 atomics).  NULL = energy only.  Zeroed by the library.
 * CSR when neighbor_ptr != NULL (idx_j = neighbor_list[1]); otherwise a [n_atoms,max_neighbors] matrix whose entries
 * j >= fill_value or j >= n_atoms are padding (:325).  energy_prefactor is 0.5 for every reference kernel except the energy-only
 * matrix kernels, which omit the 1/2 (:340, :623): the caller passes 1.0 for those to stay result-identical.
 * mi_coulomb_bwd is the adjoint of `energies` for L = sum_i g_i E_i w.r.t. positions / charges / cell (replaces the Warp-tape
 * backward, coulomb.py:716-1330 via autograd.py:525-665); outputs float64, zeroed by the library.                           */
int mi_coulomb(const double* positions, const double* charges, const double* cell /*[n_systems,3,3]*/, const int32_t* batch_idx,
               int n_atoms, const int32_t* idx_j, const int32_t* unit_shifts, const int32_t* neighbor_ptr, int max_neighbors,
               int fill_value, double cutoff, double alpha, double energy_prefactor, double* energies /*[n_atoms]*/,
               double* forces /*[n_atoms,3] or NULL*/, void* stream);
int mi_coulomb_bwd(const double* positions, const double* charges, const double* cell, const int32_t* batch_idx, int n_atoms,
                   int n_systems, const int32_t* idx_j, const int32_t* unit_shifts, const int32_t* neighbor_ptr, int max_neighbors,
                   int fill_value, double cutoff, double alpha, double energy_prefactor, const double* grad_energies /*[n_atoms]*/,
                   double* grad_positions /*[n_atoms,3]*/, double* grad_charges /*[n_atoms]*/, double* grad_cell /*[n_systems,3,3]*/,
                   void* stream);

/* Adjoint of the `forces` output for L = sum_k grad_forces_k . F_k (the reference lists `forces` in the ops' grad_arrays, coulomb.py:785-790,
 * :937-945 and replays its tape): second derivatives of the pair term, entry-wise scatter, any list; outputs float64, zeroed by the library. */
int mi_coulomb_forces_bwd(const double* positions, const double* charges, const double* cell, const int32_t* batch_idx, int n_atoms,
                          int n_systems, const int32_t* idx_j, const int32_t* unit_shifts, const int32_t* neighbor_ptr, int max_neighbors,
                          int fill_value, double cutoff, double alpha, const double* grad_forces /*[n_atoms,3]*/,
                          double* grad_positions /*[n_atoms,3]*/, double* grad_charges /*[n_atoms]*/, double* grad_cell /*[n_systems,3,3]*/,
                          void* stream);

/* ---- B-spline spread / gather ---------------------------------------------------------------
 * Replaces alchemiops::_[batch_]spline_spread / _gather / _gather_vec3 (spline.py:1500-2107; kernels
 * :497-676, :763-959).  Orders 1-4 use the reference's piecewise polynomials; orders 5-6 use the true
 * cardinal B-spline recursion (the reference returns 0 there: SURVEY F2).  mesh is [n_systems,nx,ny,nz].
 * `batched` selects the reference's batch-kernel weight threshold (w > 1e-8 instead of w > 0 in spread).
 *
 * Every `order` argument below may carry MI_SPLINE_REFERENCE_ORDERS: orders 5 and 6 are then evaluated as the reference evaluates them --
 * all weights ZERO (spline.py:150-193 implements orders 1-4 only: spread leaves a zero mesh, every gather returns zeros) and the
 * structure-factor exponent capped at 4 (pme_kernels.py:213-225) -- instead of as true B-splines with exponent = order.  Orders 1-4 are
 * the same either way.  The host API sets the bit per call (nvalchemiops.spline.reference_spline_orders); no library state is involved.
 */
#define MI_SPLINE_REFERENCE_ORDERS 0x100
/* Per-system cell geometry for the mesh ops in one launch: cell_inv_t = (cell^-1)^T, reciprocal_cell = 2 pi cell^-1, volume = |det|
 * (the torch.linalg.inv_ex / det calls of `_pme_reciprocal_space_impl`, pme.py:1382-1395).  All [n_systems,...] in `dtype`.       */
int mi_cell_geometry(const void* cell, int n_systems, int dtype, void* cell_inv_t, void* reciprocal_cell, void* volume, void* stream);
/* The same plus total_charge[s] = sum of the charges of system s (charges.sum() / scatter_add_, pme.py:1225,1241-1244) in ONE launch
 * (total_charge is zeroed by the library): everything the fused PME step needs before the spread.                                  */
int mi_pme_prepare(const void* cell, const void* charges, const int32_t* batch_idx, int n_atoms, int n_systems, int dtype,
                   void* cell_inv_t, void* reciprocal_cell, void* volume, void* total_charge /*[n_systems]*/, void* stream);
/* 1 when mi_spline_spread (given its workspace) runs tile-owned for this mesh / order: every mesh point is then written, so the
 * caller may skip the zero-fill of `mesh`.                                                                                          */
int mi_spline_spread_is_tiled(int n_systems, int nx, int ny, int nz, int order);
/* 1 when the tile-owned run is also the FASTER one for this atom count (host policy: >= 12 000 atoms and >= 128 mesh tiles over all systems;
 * below that the zero-fill + atomic kernel + per-atom gather cost fewer launches).  A caller that follows it passes workspace = NULL (and a
 * zeroed mesh, and spread_workspace = NULL to mi_pme_gather_finish) when this returns 0.                                                   */
int mi_spline_spread_prefers_tiles(int n_atoms, int n_systems, int nx, int ny, int nz, int order);
int mi_spline_spread(const void* positions, const void* values, const int32_t* batch_idx,
                     const void* cell_inv_t /*[n_systems,3,3]*/, int n_atoms, int n_systems, int nx, int ny,
                     int nz, int order, int batched, int dtype, void* mesh /* zeroed by caller unless mi_spline_spread_is_tiled */,
                     void* workspace /* mi_spline_spread_workspace_bytes, or NULL */, size_t workspace_bytes, void* stream);
/* With a workspace the spread runs tile-owned when every mesh dimension has a divisor e with max(order - 1, 2) <= e <= 8 (atoms
 * binned by ex*ey*ez mesh tile, LDS accumulation, every mesh point written once, no global atomics); otherwise order^2 threads per
 * atom add into the zeroed mesh.                                                                                               */
size_t mi_spline_spread_workspace_bytes(int n_atoms, int n_systems, int nx, int ny, int nz);
/* The exact size for one (order, dtype): the tile-box scratch, by far the largest part, is (e + order - 1)^3 values of the mesh dtype per
 * tile instead of the any-order fp64 bound above (256^3, fp32, order 4: 178 MB instead of 576).  mi_spline_spread accepts either size.   */
size_t mi_spline_spread_workspace_bytes_for(int n_atoms, int n_systems, int nx, int ny, int nz, int order, int dtype);
/* byte offset, inside the workspace mi_spline_spread was given, of int32[4 + n_atoms] that the tile-owned spread leaves behind (valid until
 * the workspace is reused): [0] = number of consecutive atom pairs (i, i+1) that sit in neither the same nor neighbouring mesh tiles (a
 * measure of how spatially incoherent the caller's atom order is), [1..3] unused, [4..] = the atom ids grouped by mesh tile.
 * -1 when this mesh / order runs the atomic kernel, which does not sort. */
long long mi_spline_spread_order_offset(int n_atoms, int n_systems, int nx, int ny, int nz, int order);
/* channels = 1: out[n_atoms] += sum_g mesh[g] w ; channels = 3 (mesh [..,3] interleaved) or 4 planar:
 * see mi_pme_gather below for the fused PME form.                                                     */
int mi_spline_gather(const void* positions, const void* mesh, const int32_t* batch_idx, const void* cell_inv_t,
                     int n_atoms, int n_systems, int nx, int ny, int nz, int order, int dtype,
                     void* out /*[n_atoms]*/, void* stream);
int mi_spline_gather_vec3(const void* positions, const void* charges, const void* mesh_vec3 /*[B,nx,ny,nz,3]*/,
                          const int32_t* batch_idx, const void* cell_inv_t, int n_atoms, int n_systems, int nx,
                          int ny, int nz, int order, int dtype, void* out /*[n_atoms,3]*/, void* stream);

/* Gradient of a gather w.r.t. the fractional coordinate: out[i][a] = sum_g mesh[g] * d w_i(g) / d frac_a  (frac = cell_inv_t . r;
 * the factor mesh_dims[a] of d theta / d frac is included).  Building block of the spread / gather adjoints
 * (reference: _bspline_gather_gradient_kernel, spline.py:680-760, and the Warp adjoints of the spread/gather kernels).      */
int mi_spline_gather_grad(const void* positions, const void* mesh, const int32_t* batch_idx, const void* cell_inv_t, int n_atoms,
                          int n_systems, int nx, int ny, int nz, int order, int dtype, void* out /*[n_atoms,3]*/, void* stream);

/* Second-order building blocks: the adjoint of `spline_gather_gradient` (alchemiops::_[batch_]spline_gather_gradient lists positions,
 * charges, mesh and cell_inv_t in its grad_arrays, spline.py:1750-1840, :2110-2200; the reference replays its Warp tape).  With
 * W_i(g) the 3-D weight of atom i at mesh point g and frac = cell_inv_t . r (derivatives include the mesh_dims factors):
 *   mi_spline_gather_hess_dot  out[i][b] = sum_g mesh[g] sum_a vec[i][a] d^2 W_i(g) / dfrac_a dfrac_b
 *   mi_spline_spread_grad      mesh[g]   = sum_i sum_a vec[i][a] d W_i(g) / dfrac_a          (mesh is zeroed by the call)        */
int mi_spline_gather_hess_dot(const void* positions, const void* mesh, const int32_t* batch_idx, const void* cell_inv_t,
                              const void* vec /*[n_atoms,3]*/, int n_atoms, int n_systems, int nx, int ny, int nz, int order, int dtype,
                              void* out /*[n_atoms,3]*/, void* stream);
int mi_spline_spread_grad(const void* positions, const void* vec /*[n_atoms,3]*/, const int32_t* batch_idx, const void* cell_inv_t,
                          int n_atoms, int n_systems, int nx, int ny, int nz, int order, int dtype, void* mesh /*[B,nx,ny,nz]*/,
                          void* stream);

/* ---- multi-channel spread / gather: values[n_atoms, C] (row major) <-> mesh[n_systems, C, nx, ny, nz] (planar channels) -------------
 * Replace alchemiops::_[batch_]spline_spread_channels / _gather_channels (spline.py:2202-2580; kernels :1053-1330): the multipole path,
 * C = 9 for L_max = 2.  The channels share stencil, tile and 1-D weights; only the per-atom value differs, so the tile path runs the key
 * kernel and the counting sort ONCE and accumulates a block of channels per box kernel (as many LDS boxes as fit 48 KiB, at most 9),
 * box + reduce once per block; the atomic path evaluates the weights once and loops over the channels.  Weight thresholds are those of
 * mi_spline_spread (w > 0, batched: w > 1e-8), any C >= 1.  Unlike mi_spline_spread the call WRITES the whole mesh on either path (the
 * atomic path zero-fills it first): the caller's mesh may be uninitialised.  Tiles run when `workspace` holds
 * mi_spline_spread_channels_workspace_bytes_for(...) bytes and the mesh tiles (mi_spline_spread_is_tiled); NULL selects the atomic path. */
size_t mi_spline_spread_channels_workspace_bytes_for(int n_atoms, int n_systems, int nx, int ny, int nz, int order, int n_channels, int dtype);
int mi_spline_spread_channels(const void* positions, const void* values /*[n_atoms,C]*/, const int32_t* batch_idx, const void* cell_inv_t,
                              int n_atoms, int n_systems, int n_channels, int nx, int ny, int nz, int order, int batched, int dtype,
                              void* mesh /*[n_systems,C,nx,ny,nz]*/, void* workspace, size_t workspace_bytes, void* stream);
/* out[i][c] = sum_g mesh[c][g] w_i(g), weights <= 1e-8 skipped: per channel the very operations of mi_spline_gather, in its order, so
 * a channel equals the scalar gather of its plane bit for bit.                                                                        */
int mi_spline_gather_channels(const void* positions, const void* mesh /*[n_systems,C,nx,ny,nz]*/, const int32_t* batch_idx,
                              const void* cell_inv_t, int n_atoms, int n_systems, int n_channels, int nx, int ny, int nz, int order, int dtype,
                              void* out /*[n_atoms,C]*/, void* stream);
/* out[i][a] = sum_c coef[i][c] sum_g mesh[c][g] d w_i(g) / d frac_a: mi_spline_gather_grad over the channels, weighted per atom and
 * channel -- the position / cell branch of both adjoints (spread: mesh = grad_mesh, coef = values; gather: mesh = mesh, coef = grad_out). */
int mi_spline_gather_channels_frac_grad(const void* positions, const void* mesh /*[n_systems,C,nx,ny,nz]*/, const void* coef /*[n_atoms,C]*/,
                                        const int32_t* batch_idx, const void* cell_inv_t, int n_atoms, int n_systems, int n_channels, int nx,
                                        int ny, int nz, int order, int dtype, void* out /*[n_atoms,3]*/, void* stream);

/* ---- multipole basis functions (csrc/multipole.hip), float64, L_max in {0, 1, 2} -> 1 / 4 / 9 components -------------------------
 * Host-callable counterparts of the reference's math/spherical_harmonics.py and math/gto.py wrappers (eval_*_pytorch).  Real
 * orthonormal harmonics of r / |r| in the order [Y00, Y1-1 (y), Y10 (z), Y1+1 (x), Y2-2 (xy), Y2-1 (yz), Y20, Y2+1 (xz), Y2+2 (x^2-y^2)],
 * 1 / r = rsqrt(r^2 + 1e-30).  out is row-major [n, components]; the gradient [n, components, 3] is d Y_lm(r / |r|) / d r.
 *   mi_gto_density   sqrt(4 pi) / (2 pi sigma^2)^(3/2) Y_lm(r^) exp(-r^2 / (2 sigma^2))
 *   mi_gto_fourier   exp(-k^2 sigma^2 / 2) x {1 (L = 0, real), (1/2) sqrt(4 pi) Y_1m(k^) (L = 1, imaginary), -(1/4) sqrt(4 pi) Y_2m(k^)
 *                    (L = 2, real)}; the other part is written as zero.                                                             */
int mi_sph_harm(const double* positions /*[n,3]*/, int n, int l_max, double* out, void* stream);
int mi_sph_harm_grad(const double* positions /*[n,3]*/, int n, int l_max, double* out, void* stream);
int mi_gto_density(const double* positions /*[n,3]*/, int n, double sigma, int l_max, double* out, void* stream);
int mi_gto_fourier(const double* k_vectors /*[n,3]*/, int n, double sigma, int l_max, double* out_real, double* out_imag, void* stream);

/* ---- FFT plans (csrc/fft.cpp: hipFFT on rocFFT) ------------------------------------------------------------------------
 * 3-D real <-> complex transforms over a batch of contiguous meshes: real [batch][nx][ny][nz], complex [batch][nx][ny][nz/2+1]
 * interleaved.  Replace torch.fft.rfftn(norm="backward") / irfftn(norm="forward") of `_pme_reciprocal_space_impl` (pme.py:1398,
 * :1422, :1455-1457): both directions UNSCALED.  `inverse` = 0: R2C forward, 1: C2R inverse -- which may OVERWRITE its input
 * spectrum (rocFFT's multi-dimensional C2R; this is why torch clones before irfftn -- here the spectrum is scratch of the same step).
 * A plan owns its work area (mi_fft_plan_work_bytes, allocated at creation on the then-current device): the one object of this ABI
 * that holds device memory.  mi_fft_plan_exec allocates nothing, never synchronises, is HIP-graph capturable.                     */
int mi_fft_plan_create(int nx, int ny, int nz, int batch, int dtype, int inverse, void** plan_out);
size_t mi_fft_plan_work_bytes(const void* plan);
int mi_fft_plan_exec(void* plan, void* in, void* out, void* stream);
int mi_fft_plan_destroy(void* plan);

/* hipFFT versions as major * 10000 + minor * 100 + patch: compiled-against and loaded at run time (they can differ inside a Python process,
 * where torch has already loaded its own copy of the same SONAME).                                                                  */
int mi_fft_library_versions(int* compiled, int* loaded);

/* ---- dense DFT (csrc/dft.hip) -------------------------------------------------------------------------------------------
 * The same transforms as mi_fft_plan_exec -- real [batch][nx][ny][nz] <-> complex [batch][nx][ny][nz/2+1], both directions unscaled --
 * for ANY mesh size, evaluated from the definition (three passes of 1-D DFTs, each split once into two dense levels, n1 + n2 multiply-adds
 * per output; sincospi twiddles in double): no plan, no library
 * behind it, no state.  O(sqrt n) per output: this is the transform of last resort, used when a hipFFT plan fails its known-answer test at
 * creation (rocFFT on this stack can return a wrong transform for some shapes depending on what the process planned before),
 * and the cross-check of every other FFT path in the tests.  inverse != 0: `in` (complex) is transformed in place along x and y before
 * the z pass writes `out` -- it is scratch, as for hipFFT's multi-dimensional C2R.  Replaces torch.fft.rfftn / irfftn of
 * interactions/electrostatics/pme.py:1398, :1422, :1455-1457 on that path.                                                          */
#define MI_DFT_MAX_N 1024
int mi_dft3d(void* in, void* out, int nx, int ny, int nz, int batch, int dtype, int inverse, void* stream);

/* ---- PME reciprocal-space mesh kernels ------------------------------------------------------
 * mi_pme_green_sf: alchemiops::_[batch_]pme_green_structure_factor (pme.py:273-553, pme_kernels.py:121-331)
 * mi_pme_convolve: the torch elementwise block of _pme_reciprocal_space_impl (pme.py:1418-1419,1455-1457):
 *   conv = spec / sf2 * G ; E_d = -i k_d conv, fused into one pass that writes 1 or 4 spectra.  k and k^2 are evaluated in registers
 *   from recip_cell unless the caller's precomputed arrays are passed (pme_reciprocal_space(k_vectors=, k_squared=), pme.py:1386-1392).
 *   exponent of the sinc product before squaring, in both: `order` (true order-5/6 splines), or min(order, 4) as in the reference
 *   (pme_kernels.py:213-225) when `order` carries MI_SPLINE_REFERENCE_ORDERS.
 * mi_pme_gather_finish: spline_gather + pme_energy_corrections[_with_charge_grad] + gather_vec3 + "x2"
 *   (pme.py:1429-1477; pme_kernels.py:340-657) fused over the 4 planar real-space meshes.  add_energies / add_forces /
 *   add_charge_grads (NULL ok): the real-space part (mi_ewald_real outputs: float64 energies and charge gradients, forces in
 *   `dtype`) added in the epilogue -- the `real + reciprocal` sums of particle_mesh_ewald (pme.py:1975-1990).
 *   spread_workspace selects the tile-staged kernel (round 4); results equal the per-atom kernel's up to the order of the order^3 additions.
 */
int mi_pme_green_sf(const void* k_squared /*[B,nx,ny,nzr]*/, const void* alpha /*[B]*/, const void* volume /*[B]*/,
                    int n_systems, int nx, int ny, int nz, int sf_exponent, int dtype, void* green /*[B,nx,ny,nzr]*/,
                    void* sf_sq /*[nx,ny,nzr]*/, void* stream);
int mi_pme_convolve(const void* spec /*complex [B,nx,ny,nzr]*/, const void* recip_cell /*[B,3,3] = 2pi inv(cell)*/,
                    const void* alpha /*[B]*/, const void* volume /*[B]*/, int n_systems, int nx, int ny, int nz,
                    int sf_exponent, int with_field, int dtype,
                    const void* k_vectors /*[(B,)nx,ny,nzr,3] or NULL*/, const void* k_squared /*[(B,)nx,ny,nzr] or NULL*/,
                    int k_batched /*the k arrays carry a leading system dimension*/, void* out /*complex [B,(1|4),nx,ny,nzr]*/, void* stream);
/* Fused mesh solve: everything between the spread and the gather of pme.py:1398-1461 -- rfftn, (spec / sf^2) G, the three field spectra
 * -i k_d conv, and the four inverse transforms (norm="forward": unscaled) -- for a mesh whose sizes are products of 2, 3 and 5 (round 6: mixed-radix lines; powers of two only before), in four kernels (+ one tiny table
 * launch into the scratch) that keep a whole (y,z) plane resp. 16 x-columns in LDS (csrc/fft_lds.h): mesh [n_systems][nx][ny][nz] real -> real_out [n_systems][1|4][nx][ny][nz]
 * (potential, then E_x, E_y, E_z when with_field), exactly what mi_fft_plan_exec (R2C) -> mi_pme_convolve -> mi_fft_plan_exec (C2R) leave,
 * without the charge spectrum as a by-product (callers that need it -- the adjoint of the autograd node -- keep the three-call form, or
 * mi_pme_solve_keep below).  No state outlives the call.
 * The inverse follows numpy / torch irfftn in not reading the imaginary parts of the DC and Nyquist bins along z.
 * supported: nx, ny in {8..256}, nz in {8..512} and even, every size a product of 2, 3 and 5 (96, 100, 120 ... as well as the powers of two), one (ny, nz/2+1) complex plane + its tables within 160 KB of LDS
 * (fp64: 128 x 128, 64 x 256; fp32: 256 x 128, 128 x 256).  k is evaluated from recip_cell (2 pi cell^-1, mi_pme_prepare).            */
int mi_pme_solve_supported(int n_systems, int nx, int ny, int nz, int dtype);
/* 1 when the fused solve is the path to take (host policy, measured: since round 5 wherever it is supported -- at parity with hipFFT's
 * batched plans for batches of small meshes, ahead for single and large meshes, and independent of rocFFT) */
int mi_pme_solve_preferred(int n_systems, int nx, int ny, int nz, int dtype);
size_t mi_pme_solve_scratch_bytes(int n_systems, int nx, int ny, int nz, int n_channels /*1 | 4*/, int dtype);
int mi_pme_solve(const void* mesh, const void* recip_cell /*[n_systems,3,3]*/, const void* alpha /*[n_systems]*/,
                 const void* volume /*[n_systems]*/, int n_systems, int nx, int ny, int nz, int order /* as mi_pme_convolve */,
                 int with_field, int dtype, void* scratch, size_t scratch_bytes, void* real_out, void* stream);
/* The same, and additionally the charge spectrum itself: spectrum_out (NULL ok) [n_systems][nx][ny][nz/2+1] complex, UNSCALED forward
 * transform of `mesh` in natural frequency order -- what mi_fft_plan_exec (R2C) / torch.fft.rfftn leave -- written by the forward column
 * kernel as a by-product (one 16-byte store per bin).  For callers that need it later (the backward of the autograd node).  Prepared at the
 * end of round 4: index arithmetic checked on the host (tests/test_fft_lds_cpu.py), not yet run or timed on a GPU; the Python host code
 * uses it only under NVALCHEMIOPS_PME_SOLVE_AUTOGRAD=1.                                                                                  */
int mi_pme_solve_keep(const void* mesh, const void* recip_cell, const void* alpha, const void* volume, int n_systems, int nx, int ny, int nz,
                      int order, int with_field, int dtype, void* scratch, size_t scratch_bytes, void* real_out, void* spectrum_out,
                      void* stream);
/* The mesh solve's kernels as 3-D transforms on their own (round 6): real [batch][nx][ny][nz] <-> half spectrum [batch][nx][ny][nz/2+1]
 * (interleaved re, im; natural frequency order), UNSCALED in both directions -- layout and scaling of mi_fft_plan_exec / of
 * torch.fft.rfftn(norm="backward") and irfftn(norm="forward") (pme.py:1398, :1422, :1455-1457) -- without hipFFT: inverse = 0: plane kernel +
 * column kernel (R2C), inverse = 1: column kernel + plane kernel (C2R; like numpy / torch it does not read the imaginary parts of the DC
 * and Nyquist bins along z, and unlike hipFFT's multi-dimensional C2R it leaves its input untouched).  Supported
 * (mi_fft_lds_supported) where mi_pme_solve_supported(batch, nx, ny, nz, dtype) is and the plane kernel's two extra index tables still fit.  scratch: mi_fft_lds_scratch_bytes (one half spectrum + the per-shape tables);
 * nothing outlives the call, nothing is allocated or synchronised: capturable in a HIP graph.  The backward of the autograd node, the
 * composed differentiable path and the spectrum-keeping callers take these instead of a hipFFT plan wherever the mesh allows.          */
int mi_fft_lds_supported(int batch, int nx, int ny, int nz, int dtype);
size_t mi_fft_lds_scratch_bytes(int batch, int nx, int ny, int nz, int dtype);
int mi_fft_lds(const void* in, void* out, int batch, int nx, int ny, int nz, int dtype, int inverse, void* scratch, size_t scratch_bytes,
               const void* tables /*NULL, or a block filled by mi_fft_lds_tables for this (nx, ny, nz, dtype)*/, void* stream);
/* The per-shape tables of the in-LDS kernels (unit roots, Miller index and sinc of every slot: a few KB; they depend on nx, ny, nz and the
 * dtype only).  Every call of mi_fft_lds / mi_pme_solve* computes them into its scratch with one small launch unless the caller passes a
 * block it filled ONCE with mi_fft_lds_tables -- caller-owned memory, read-only afterwards, shareable by any number of calls and streams
 * once that launch has completed (saves ~6 us per call: the Python host keeps one block per mesh shape and device).                       */
size_t mi_fft_lds_tables_bytes(int nx, int ny, int nz, int dtype);
int mi_fft_lds_tables(int nx, int ny, int nz, int dtype, void* tables, void* stream);
/* mi_pme_solve_keep with the tables handed in (NULL = computed by the call, as in mi_pme_solve / mi_pme_solve_keep) */
int mi_pme_solve_tabled(const void* mesh, const void* recip_cell, const void* alpha, const void* volume, int n_systems, int nx, int ny, int nz,
                        int order, int with_field, int dtype, void* scratch, size_t scratch_bytes, void* real_out, void* spectrum_out,
                        const void* tables, void* stream);
/* Adjoint of the k-space pass (the backward of the fused forward under autograd, pme.py `_FusedPME` / `_FusedReciprocal`).  `spec`: unscaled
 * spectrum of the charge mesh [n_systems][nx][ny][nz/2+1]; `weight_spec`: spectra of the spread upstream weights, channel-major
 * [n_channels][n_systems][...] -- channel 0 for a loss on the energies (weights g_E q), channels 1..3 (n_channels = 4) for a loss on the explicit
 * forces (weights 2 g_F,d q).  Writes conv_out = D (A_E_hat + sum_d i k_d A_d_hat), whose unscaled inverse transform is dL/d(charge mesh), and per
 * system and block 20 sums: {-V dL/dV, dL/dalpha, dL/d(2 pi cell^-1)[3][3] through k^2, the same through the explicit k_d of the field}: closed
 * form of what the reference's Warp tape + torch autograd produce for pme_kernels.py:121-331 / pme.py:1398-1457.  partial:
 * [n_systems][mi_pme_convolve_bwd_blocks()][20] doubles, every entry written; the caller folds the block dimension.                     */
int mi_pme_convolve_bwd(const void* spec, const void* weight_spec, int n_channels, const void* recip_cell, const void* alpha, const void* volume,
                        int n_systems, int nx, int ny, int nz, int order, int dtype, void* conv_out, double* partial, void* stream);
int mi_pme_convolve_bwd_blocks(void);
/* Virial of the mesh sum from the charge spectrum `spec` [B,nx,ny,nzr] (the unscaled R2C of the spread charges, as the k-space step holds it):
 *   W[a][b] = sum_m h_m E_m (delta_ab - 2 (1/k^2 + 1/(4 alpha^2)) k_a k_b),  E_m = G(k_m) |spec_m|^2 / sf2_m,  h = 1 on kz = 0 and the
 * Nyquist plane, else 2 -- -dE/d(strain) at fixed alpha, mesh and order.  k from recip_cell (2 pi cell^-1), or from the caller's k_vectors
 * [(B,)nx,ny,nzr,3] and k_squared [(B,)nx,ny,nzr] (both or neither; k_batched = 1: with the leading system dimension).  Six sums {xx, yy, zz,
 * xy, xz, yz} per system and block: partial [n_systems][mi_pme_virial_blocks()][6] float64, every entry written, the caller folds the blocks.
 * total_charge [n_systems] in `dtype` (NULL: left out): the background term -pi Q^2 / (2 alpha^2 V) joins the diagonal (it scales as 1/V).     */
int mi_pme_virial(const void* spec, const void* recip_cell, const void* alpha, const void* volume, int n_systems, int nx, int ny, int nz, int order,
                  int dtype, const void* k_vectors, const void* k_squared, int k_batched, const void* total_charge, double* partial, void* stream);
int mi_pme_virial_blocks(void);

/* Particle-mesh Ewald for point dipoles (csrc/pme.hip, last section; driver: nvalchemiops/interactions/electrostatics/pme_dipole.py): smooth PME
 * with analytic spline derivatives.  With W_i(g) the order-p B-spline weight of atom i at mesh point g (as mi_spline_spread places it), grad the
 * Cartesian gradient w.r.t. r_i (d W / d r_b = sum_a cit[a][b] n_a d W / d m_a, cit = cell_inv_t) and c = 2 alpha^3 / (3 sqrt(pi)):
 *     rho_q = sum_i q_i W_i,  rho_mu = sum_i mu_i . grad W_i,  phi_X = the mesh solve of rho_X (mi_pme_solve* with_field = 0, or R2C ->
 *     mi_pme_convolve -> C2R: linear, so the meshes are further systems of one batched call),  phi_t = phi_q + phi_mu,
 *     E_i = q_i W_i.phi_mu + mu_i.grad W_i.phi_t - c |mu_i|^2
 * order is 4, 5 or 6 (the plain order: MI_SPLINE_REFERENCE_ORDERS is refused), every mesh dimension >= order; positions, charges, dipoles
 * [n_atoms][3], cell_inv_t, alpha and the meshes are in `dtype`; weights, where given, are float64 [n_atoms].
 *
 * mi_pme_dipole_spread: one pass over the atoms (order^2 threads each) adds q_i W_i into meshes[0] and mu_i . grad W_i into meshes[1], and with
 * weights g also g_i q_i W_i into meshes[2] and g_i mu_i . grad W_i into meshes[3]: meshes [2 (weights NULL) | 4][n_systems][nx][ny][nz], ZEROED BY
 * THIS CALL.  Floating-point atomic adds: a mesh is reproducible up to the arrival order of its adds only.
 *
 * mi_pme_dipole_gather: one read of mesh_a and mesh_b [n_systems][nx][ny][nz] per stencil point gives, per atom,
 *     D_i = { dq: W_i.A,  dmu: grad W_i.B,  dr: q_i grad W_i.A + (mu_i . grad) grad W_i.B }
 * and writes charge_grads[i] = s_i D_i.dq, dipole_grads[i] = s_i D_i.dmu - 2 c w_i mu_i, forces[i] = -s_i D_i.dr (positions dtype; the others
 * float64), with s_i = 2, w_i = 1 (weights NULL: the forward call over (A, B) = (phi_mu, phi_t), every atom being source and probe) or
 * s_i = w_i = weights[i] (the first launch of the adjoint of L = sum_i g_i E_i, same meshes).  accumulate = 1 (weights must be NULL): s_i = 1, no
 * self term, and the three outputs are ADDED to what they hold -- the second launch of the adjoint, over (A, B) = (phi^g_mu, phi^g_q + phi^g_mu)
 * of the weighted meshes.  energies[i] (float64) = q_i W_i.A + mu_i . grad W_i.B - c |mu_i|^2, never weighted or accumulated.  Any output may be
 * NULL.  No atomics.
 *
 * mi_pme_dipole_virial: the k-space part of -dE/d(strain) from the two spectra [n_systems][nx][ny][nzr] (unscaled R2C of rho_q and rho_mu),
 *     W[a][b] = sum_m h_m E_m (delta_ab - 2 (1/k^2 + 1/(4 alpha^2)) k_a k_b),  E_m = G(k_m) (2 Re[conj(spec_q) spec_mu] + |spec_mu|^2) / sf2_m,
 * h as for mi_pme_virial.  Nine sums (row-major 3 x 3) per system and block: partial [n_systems][mi_pme_dipole_virial_blocks()][9] float64, every
 * entry written, the caller folds the blocks AND adds the term of the dipoles' fractional components, which follow the strain while the dipoles
 * stay fixed in the laboratory frame: sum_i (dE/dmu_i without its self term)[a] mu_i[b] per system (in this index order; it makes the virial
 * non-symmetric). */
int mi_pme_dipole_spread(const void* positions, const void* charges, const void* dipoles, const double* weights, const int32_t* batch_idx,
                         const void* cell_inv_t, int n_atoms, int n_systems, int nx, int ny, int nz, int order, int dtype, void* meshes, void* stream);
int mi_pme_dipole_gather(const void* positions, const void* charges, const void* dipoles, const double* weights, const int32_t* batch_idx,
                         const void* cell_inv_t, const void* mesh_a, const void* mesh_b, const void* alpha /*[n_systems]*/, int n_atoms, int n_systems,
                         int nx, int ny, int nz, int order, int dtype, int accumulate, double* energies, void* forces, double* charge_grads,
                         double* dipole_grads, void* stream);
int mi_pme_dipole_virial(const void* spec_q, const void* spec_mu, const void* recip_cell, const void* alpha, const void* volume, int n_systems, int nx,
                         int ny, int nz, int order, int dtype, double* partial, void* stream);
int mi_pme_dipole_virial_blocks(void);

/* Particle-mesh Ewald for point quadrupoles (csrc/pme.hip, last section; driver: nvalchemiops/interactions/electrostatics/pme_quadrupole.py): the
 * dipole section continued by one multipole order.  quadrupoles [n_atoms][3][3] in `dtype`, 1/2 (Q + Q^T) of it is used; l_i = q_i + mu_i . grad,
 * Theta_i = Q_i : grad grad, c3 = 4 alpha^3 / (3 sqrt(pi)), c5 = 4 alpha^5 / (5 sqrt(pi)):
 *     rho_l = sum_i l_i W_i,  rho_T = sum_i Theta_i W_i,  phi_T = the mesh solve of rho_T,  phi_L = the mesh solve of rho_l, plus phi_T,
 *     E_i = l_i W_i.phi_T + Theta_i W_i.phi_L + c3 q_i tr Q_i - c5 (2 Q_i:Q_i + (tr Q_i)^2)
 * order is 5 or 6 (the forces need the third derivative of the spline, which is not continuous at order 4); everything else as for mi_pme_dipole_*.
 *
 * mi_pme_quadrupole_spread: one pass over the atoms adds l_i W_i into meshes[0] and Theta_i W_i into meshes[1], and with weights g their g-weighted
 * twins into meshes[2] and meshes[3]: meshes [2 (weights NULL) | 4][n_systems][nx][ny][nz], ZEROED BY THIS CALL.  Floating-point atomic adds; a
 * value that is exactly zero is not added, so zero quadrupoles leave meshes[1] exactly zero.
 *
 * mi_pme_quadrupole_gather: one read of mesh_a and mesh_b per stencil point gives, per atom,
 *     D_i = { dq: W_i.A,  dmu: grad W_i.A,  dQ: grad grad W_i.B,  dr: q_i grad W_i.A + (mu_i . grad) grad W_i.A + (Q_i : grad grad) grad W_i.B }
 * and writes charge_grads[i] = s_i D_i.dq + w_i c3 tr Q_i, dipole_grads[i] = s_i D_i.dmu, quadrupole_grads[i] (3 x 3, symmetric) = s_i D_i.dQ +
 * w_i (c3 q_i I - c5 (4 Q_i + 2 tr Q_i I)), forces[i] = -s_i D_i.dr (positions dtype; the others float64), with s_i and w_i as for
 * mi_pme_dipole_gather: 2 and 1 for the forward call over (A, B) = (phi_T, phi_L); weights[i] for the first launch of the adjoint; accumulate = 1
 * (weights NULL): s_i = 1, no self terms, outputs ADDED to what they hold -- the second launch of the adjoint, over (phi^g_T, phi^g_l + phi^g_T).
 * energies[i] (float64) = l_i W_i.A + Theta_i W_i.B + the self terms, never weighted or accumulated.  Any output may be NULL; the third-derivative
 * work is compiled only into the variant that runs when forces is given.  No atomics.
 *
 * mi_pme_quadrupole_virial: mi_pme_dipole_virial over the spectra of (rho_l, rho_T), E_m = G(k_m) (2 Re[conj(spec_l) spec_t] + |spec_t|^2) / sf2_m:
 * partial [n_systems][mi_pme_quadrupole_virial_blocks()][9] float64.  The caller folds the blocks and adds the terms of the multipoles' fractional
 * components, sum_i (dE/dmu_i)[a] mu_i[b] + 2 sum_i (G_i Q_i)[a][b] per system, G_i = dE/dQ_i without its self terms. */
int mi_pme_quadrupole_spread(const void* positions, const void* charges, const void* dipoles, const void* quadrupoles, const double* weights,
                             const int32_t* batch_idx, const void* cell_inv_t, int n_atoms, int n_systems, int nx, int ny, int nz, int order, int dtype,
                             void* meshes, void* stream);
int mi_pme_quadrupole_gather(const void* positions, const void* charges, const void* dipoles, const void* quadrupoles, const double* weights,
                             const int32_t* batch_idx, const void* cell_inv_t, const void* mesh_a, const void* mesh_b, const void* alpha /*[n_systems]*/,
                             int n_atoms, int n_systems, int nx, int ny, int nz, int order, int dtype, int accumulate, double* energies, void* forces,
                             double* charge_grads, double* dipole_grads, double* quadrupole_grads, void* stream);
int mi_pme_quadrupole_virial(const void* spec_l, const void* spec_t, const void* recip_cell, const void* alpha, const void* volume, int n_systems,
                             int nx, int ny, int nz, int order, int dtype, double* partial, void* stream);
int mi_pme_quadrupole_virial_blocks(void);

int mi_pme_gather_finish(const void* positions, const void* charges, const int32_t* batch_idx, const void* cell_inv_t,
                         const void* meshes /*[B,(1|4),nx,ny,nz] real*/, const void* alpha, const void* volume,
                         const void* total_charge /*[B]*/, int n_atoms, int n_systems, int nx, int ny, int nz,
                         int order, int with_field, int dtype, void* energies /*[n_atoms]*/,
                         void* forces /*[n_atoms,3] or NULL*/, void* charge_grads /*[n_atoms] or NULL*/,
                         const double* add_energies, const void* add_forces, const double* add_charge_grads,
                         const void* spread_workspace /*NULL, or the workspace of the tile-owned mi_spline_spread of the SAME step (same positions,
                           mesh, order; see mi_spline_spread_is_tiled): atoms grouped by mesh tile + stencil starts + fractional offsets -> the
                           tile-staged gather (mesh boxes through LDS); NULL -> the per-atom gather*/,
                         void* stream);
int mi_pme_corrections(const void* raw, const void* charges, const int32_t* batch_idx, const void* volume,
                       const void* alpha, const void* total_charge, int n_atoms, int dtype, void* energies,
                       void* charge_grads /*NULL ok*/, void* stream);
/* per-system sum of charges (charges.sum() / scatter_add_, pme.py:1225,1241-1244); out zeroed by caller */
int mi_segment_sum(const void* values, const int32_t* batch_idx, int n_atoms, int dtype, void* out /*[B]*/, void* stream);

/* ---- local-frame multipoles (csrc/frames.hip; driver: nvalchemiops/interactions/electrostatics/frames.py) ---------------------------------
 * Per-atom local dipoles [n_atoms][3] and quadrupoles [n_atoms][3][3] (1/2 (Q + Q^T) of it is used) rotated into the laboratory frame,
 * mu = R mu_loc, Q = R Q_loc R^T, and the adjoint of that map: the torque forces on the frame-defining atoms.  frame_atoms [n_atoms][3] names
 * the (z, x, y) atoms of every atom, a slot outside [0, n_atoms) names nobody; frame_kinds [n_atoms] is 0 NONE (R = I), 1 Z_ONLY, 2 Z_THEN_X,
 * 3 BISECTOR, 4 Z_BISECT, 5 THREE_FOLD (Tinker / OpenMM's axis types; csrc/frames.hip states them), any other value is NONE.  d_a = r_a - r_i is
 * the minimum image when cell [n_systems][3][3] is given (rows are lattice vectors; batch_idx [n_atoms] selects the row, NULL: system 0), the
 * plain difference when cell is NULL.  Z_THEN_X with a y atom mirrors the local y axis when d_y . (d_z x d_x) < 0.  positions, the local
 * multipoles, cell and the incoming gradients are in `dtype`; all arithmetic is float64 and every output is rounded once.  One thread per atom,
 * mi_frame_block_threads() threads per block, no atomics: every output is bit-reproducible.  A zero or collinear pair of frame vectors gives
 * non-finite values for that atom (and, after the gather, the atoms it names) only.
 *
 * mi_frame_rotate: dipoles [n_atoms][3] and quadrupoles [n_atoms][3][3] (exactly symmetric) in `dtype`; each is written exactly when its local
 * input is given.
 *
 * mi_frame_adjoint: from dipole_grads = dL/dmu and quadrupole_grads = dL/dQ (either NULL: zero; 1/2 (g + g^T) is used) writes, per atom, the
 * record records[i] = {-sum_a dL/dd_a, dL/dd_z, dL/dd_x, dL/dd_y} ([n_atoms][4][3] float64, every word written, zeros for slots the kind does
 * not use), and when asked local_dipole_grads[i] = R^T dL/dmu, local_quadrupole_grads[i] = R^T 1/2 (g + g^T) R (float64, the mirrored
 * components with their sign) and virial_rows[i][p][q] = -sum_a (dL/dd_a)[p] d_a[q] ([n_atoms][9] float64; needs a cell): minus the strain
 * derivative of L under x -> (I + eps) x with the local multipoles held fixed.
 *
 * mi_frame_gather: out[i] = sign * (records[i][0] + sum of records[e / 4][e % 4] over e = inverse_slots[inverse_ptr[i] .. inverse_ptr[i + 1])),
 * in the stored order ([n_atoms][3] in `dtype`, which need not be the dtype of the adjoint call): sign = +1 gives dL/dr, sign = -1 the torque
 * forces.  inverse_slots [n_entries] holds, for every atom, the codes 4 * j + 1 + slot of the (atom j, slot) pairs that name it; a code outside
 * [0, 4 n_atoms) is skipped.  With virial_rows, virial_partial [n_systems][mi_frame_blocks()][9] float64 receives the fixed-order per-system
 * fold of the rows (every entry written; the caller sums the blocks). */
int mi_frame_rotate(const void* positions, const void* local_dipoles, const void* local_quadrupoles, const int32_t* frame_atoms,
                    const int32_t* frame_kinds, const void* cell, const int32_t* batch_idx, int n_atoms, int n_systems, int dtype, void* dipoles,
                    void* quadrupoles, void* stream);
int mi_frame_adjoint(const void* positions, const void* local_dipoles, const void* local_quadrupoles, const int32_t* frame_atoms,
                     const int32_t* frame_kinds, const void* cell, const int32_t* batch_idx, const void* dipole_grads,
                     const void* quadrupole_grads, int n_atoms, int n_systems, int dtype, double* records, double* local_dipole_grads,
                     double* local_quadrupole_grads, double* virial_rows, void* stream);
int mi_frame_gather(const double* records, const int32_t* inverse_ptr, const int32_t* inverse_slots, long long n_entries,
                    const double* virial_rows, const int32_t* batch_idx, int n_atoms, int n_systems, int dtype, double sign, void* out,
                    double* virial_partial, void* stream);
int mi_frame_blocks(void);
int mi_frame_block_threads(void);

/* ---- multi-GPU: the one collective of the path (csrc/comm.cpp) ------------------------------------------------------------
 * The reference has no multi-GPU code; the path shards at SYSTEM granularity -- no pair crosses systems
 * (batch_cell_list.py:448-457, dftd3.py:823,1126, spline.py:809) -- so every rank runs the kernels above on its own contiguous range of
 * systems and the only exchange is an all-gather of per-system values (D3 energies fp32, PME energies fp32 / fp64): RCCL over xGMI, one
 * rank per GPU.  Python programs use nvalchemiops.distributed (torch.distributed, backend "nccl" = RCCL); these entry points give a plain
 * C / C++ caller of this ABI the same step.  RCCL is bound at run time (the copy already loaded in the process, else librccl.so.1 from the
 * ROCm installation); MI_ECOMM if there is none.
 *   rank 0: mi_comm_unique_id(id) -> ship the MI_COMM_ID_BYTES to every rank by any host channel (MPI, a socket, a file);
 *   every rank, with its GPU current (hipSetDevice): mi_comm_init(id, ..., n_ranks, rank, &comm)   -- collective, blocks until all joined;
 *   per step: mi_comm_allgather_f32(comm, mine, all, count_per_rank, stream)  -- all[r * count .. (r + 1) * count) = rank r's `mine`;
 *             equal counts on every rank (pad ragged shards to the largest, as nvalchemiops.distributed.all_gather_system_values does);
 *             enqueued on `stream`, in order with the kernels that produced `mine`; in place when mine == all + rank * count;
 *   mi_comm_destroy(comm) after the stream has drained.                                                                            */
#define MI_COMM_ID_BYTES 128
int mi_comm_library_version(int* version /*[host] RCCL's NCCL_VERSION_CODE*/);
int mi_comm_unique_id(void* id_out /*[host] MI_COMM_ID_BYTES*/, size_t bytes);
int mi_comm_init(const void* id /*[host]*/, size_t bytes, int n_ranks, int rank, void** comm_out);
int mi_comm_size(const void* comm, int* n_ranks /*NULL ok*/, int* rank /*NULL ok*/);
int mi_comm_allgather_f32(void* comm, const float* send, float* recv /*[n_ranks * count_per_rank]*/, size_t count_per_rank, void* stream);
int mi_comm_allgather_f64(void* comm, const double* send, double* recv, size_t count_per_rank, void* stream);
int mi_comm_destroy(void* comm);

#ifdef __cplusplus
}
#endif
#endif /* NVALCHEMIOPS_HIP_H */
