/*
 * plnerf_hip_mesh.h -- EXPERIMENTAL: mesh extraction on the device (the reference's nerf_extract_mesh.py:531-593).
 *   plnerf_density_grid   one call = extract_fields: the density relu(raw[..., 3]) of ONE network on a resolution^3 lattice
 *   plnerf_mc_count / plnerf_mc_emit   indexed marching cubes of a device field
 *
 * Experimental like the other headers of this directory: the library exports these entries and the binding binds them, but
 * they are outside the registered ABI -- no PLNERF_VERSION step, and they may still change.
 *
 * Conventions: those of plnerf_hip_view.h (device pointers unless said otherwise, caller-owned memory, structs live in host
 * memory and are read during the call, the call enqueues on `stream` and returns, every argument is checked before the first
 * launch, nothing is allocated inside, nothing is waited for, no environment variable is read).
 */
#ifndef PLNERF_HIP_MESH_H
#define PLNERF_HIP_MESH_H

#include "plnerf_hip_anyview.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Values of a `stats` row of plnerf_density_grid (fp64). */
#define PLNERF_GRID_STATS 4
#define PLNERF_GRID_MIN 0
#define PLNERF_GRID_MAX 1
#define PLNERF_GRID_SUM 2
#define PLNERF_GRID_SUMSQ 3

/* Bytes of plnerf_density_grid's workspace (0: refused): the positions [rows, 3], one zero direction, the raw outputs [rows, 4]
 * and one stats partial per 1,024 rows of a block, for rows = min(max_rows, resolution^3); with a slot outside the compiled
 * trunk also the embedded rows and that route's own workspace for `rows` rows.  No pointer of `net` is followed.  256-byte
 * alignment. */
size_t plnerf_density_grid_workspace_bytes(const plnerf_anyview_net* net, int precision, int input_ch, int input_ch_views,
                                           int resolution, int max_rows);

/* field[(x res + y) res + z] = max(raw[3], 0) of the network at the point (xs[x], ys[y], zs[z]) -- extract_fields'
 * u[x, y, z] = relu(query_func(pts, 0, model)[..., 3]) -- for the whole lattice in one call.
 * net: one slot as plnerf_render_view_any takes it, dispatched the same way: FUSED = plnerf_mlp_fwd in `precision` on
 * `input_ch` | `input_ch_views` with the in-kernel encoding; CHAIN16 / LAYERS32 = plnerf_embed_rows, then plnerf_generic_fwd /
 * plnerf_generic_fwd_f32 (precision, input_ch and input_ch_views are then ignored: the slot's own hold).
 * xs, ys, zs [resolution]: the lattice's coordinates per axis, the caller's torch.linspace(bound_min[a], bound_max[a],
 * resolution) -- the library does not redo linspace's arithmetic.
 * Per block of at most max_rows consecutive lattice indices: one launch writes the block's positions into the workspace, the
 * slot's forward runs on them with a zero view direction (as the reference passes; the density head does not read the view
 * branch), one launch stores max(raw[3], 0) and the block's stats partials.  samples_per_ray of the fused forward (and of
 * plnerf_embed_rows) is the block's row count: the block is ONE ray, so every row reads the one zero direction of the
 * workspace and the entry's rule "viewdirs [n_rows / samples_per_ray, 3]" holds with one direction for any row count.
 * Rows are independent in all three routes, so the field does not depend on max_rows (but for plnerf_generic_fwd_f32's
 * k_splits remark: a layer with K >= 1,024).  A negative density is stored as +0, a NaN as NaN.
 * stats (NULL: none) [PLNERF_GRID_STATS] fp64: min, max, sum and sum of squares over the whole lattice, reduced by a last
 * one-workgroup launch in a fixed order (no floating-point atomics: the same bits on every run; the ORDER follows the blocks,
 * so sum and sum of squares may round differently for another max_rows).  min and max skip NaNs.
 * pack_weights != 0: plnerf_mlp_pack_weights of a FUSED slot first (a generic slot's weights are split in every call).
 * Only `field`, `stats` and the workspace are written (and a FUSED slot's packed buffer, a CHAIN16 slot's status word).
 * NVS networks only: input_scale 1, no density activation -- the depth-supervised variant's networks are not served.
 * PLNERF_EINVAL: NULL net, xs, ys, zs, field or workspace; a misaligned or short workspace; resolution < 2; max_rows < 1; a
 * route outside the three; for the slot what plnerf_render_view_any refuses (a FUSED slot's NULL params / packed, widths or
 * precision; a generic slot's shape, params or precision, one that lacks use_viewdirs or whose widths are not 3 + 6 L | 3 + 6 M
 * with L, M <= 16).  PLNERF_ENOSYS: an unknown precision of a FUSED slot.  PLNERF_ERANGE: resolution^3 > 2^30; a block of more
 * rows than the slot's forward takes (2^29 - 1 for FUSED; plnerf_generic_fwd / _f32's limits): lower max_rows. */
int plnerf_density_grid(const plnerf_anyview_net* net, int precision, int input_ch, int input_ch_views, int resolution,
                        const float* xs, const float* ys, const float* zs, int max_rows, int pack_weights, float* field,
                        double* stats, void* workspace, size_t workspace_bytes, plnerf_stream_t stream);

/* ---- indexed marching cubes of a device field [nx][ny][nz] fp32 (linear index (x ny + y) nz + z) at `iso` ----
 * THE LIBRARY'S CONVENTION: a corner is INSIDE when f >= iso, so a NaN is outside; a lattice edge crosses when exactly one of
 * its ends is inside.  (PyMCubes flags f < iso as far as its written description goes; neither it nor trimesh was at hand, so
 * nothing here is claimed against them.)  The case table is csrc/mc_table.h, generated by tools/gen_mc_table.py: ambiguous
 * faces cut each inside corner off separately, by a rule that reads only the face's corners.
 * Vertices: one per crossing edge, ordered by the edge's owning lattice point (the end with the smaller coordinate; by linear
 * index), then by axis 0, 1, 2.  The vertex on the edge from point p along axis a has coordinate a equal to
 * p_a + (iso - f1) / (f2 - f1), evaluated in fp64 from the two fp32 values (f1 at p), and its other two coordinates are p's
 * exact integers: INDEX coordinates.  Triangles: by cell (the linear index of its lattice point), then in table order;
 * counter-clockwise seen from outside the dense region: normals (v1 - v0) x (v2 - v0) towards decreasing field.
 * Two runs on the same field give the same bytes.
 *
 * Workspace: ONE 32-bit word per lattice point (the point's vertex offset inside its 1,024-point block and its three crossing
 * flags) plus two words per block and per 1,024 blocks (the blocks' vertex and triangle offsets; a cell's triangle offset
 * inside its block is recomputed by plnerf_mc_emit): 4.008 bytes per lattice point, the field's own size.  256-byte aligned. */
size_t plnerf_mc_workspace_bytes(int nx, int ny, int nz);

/* count -> scan -> scan, three launches (no workgroup waits for another inside a launch, no atomics): leaves the offsets in
 * the workspace and counts[0] = n_vertices, counts[1] = n_triangles (two uint32 device words).  The caller reads them back --
 * the only synchronisation, and the caller's -- and allocates.  A count that does not fit is stored as 0xFFFFFFFF.
 * PLNERF_EINVAL: NULL field, counts or workspace; a misaligned or short workspace; a size below 2; iso NaN.
 * PLNERF_ERANGE: nx ny nz > 2^30. */
int plnerf_mc_count(const float* field, int nx, int ny, int nz, double iso, void* workspace, size_t workspace_bytes,
                    uint32_t* counts, plnerf_stream_t stream);

/* After plnerf_mc_count on the same field, sizes, iso and workspace: vertices [n_vertices][3] fp64, triangles
 * [n_triangles][3] int32.  cap_vertices / cap_triangles: the rows the caller allocated -- no row at or past them is written,
 * whatever the device counts say.  Both 0: PLNERF_OK, no launch (the empty surface).  One launch.
 * PLNERF_EINVAL: as plnerf_mc_count; a negative capacity; NULL vertices / triangles with a positive capacity.
 * PLNERF_ERANGE: a capacity above 2^31 - 1 (int32 indices). */
int plnerf_mc_emit(const float* field, int nx, int ny, int nz, double iso, const void* workspace, size_t workspace_bytes,
                   double* vertices, int64_t cap_vertices, int32_t* triangles, int64_t cap_triangles, plnerf_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* PLNERF_HIP_MESH_H */
