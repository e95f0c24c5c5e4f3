// mdh_surface.h -- the kernels of mdh_surface_mesh and mdh_surface_mesh_device (mdh_api.hip): naive surface nets over a
// regular grid of the scene's distance, deterministic in values and in order.  Included by mdh_kernels.h behind k_listed,
// whose scan of listed kinds it shares; not part of the hiprtc build (built-in kinds only).
//
// THE DEFINITION (include/madarch_hip.h states it for the caller).  Every operation is one binary32 operation, unfused.
//  1. Corner (i, j, k), 0 <= i <= cx and so on, lies at p_x = origin_x + (float) i * h -- one product, then one sum --
//     likewise y and z.  Its value is v = fl (D (p) - iso): the bits mdh_contacts gives as dist at p with radius iso.  A
//     corner is INSIDE iff v < 0; zero and NaN are outside.
//  2. Cell (i, j, k), 0 <= i < cx and so on, has the corners c = 0 .. 7: bit 0 of c is the x offset, bit 1 the y offset,
//     bit 2 the z offset.  A cell is ACTIVE iff some of its corners are inside and some are outside.
//  3. The vertex of an active cell comes from its 12 edges in a fixed order: the outer loop over the axes a = x, y, z, the
//     inner loop over e = 0 .. 3, where the two other axes in ascending order take the offsets e & 1 and e >> 1.  An edge
//     CROSSES iff its endpoints v0 (offset 0 along a) and v1 differ in insideness; then t = v0 / (v0 - v1) and its local
//     point q has t on axis a and the edge's offsets 0 or 1 on the other two.  s = s + q in that order from 0 over the m
//     crossing edges, u = s / (float) m per component, and the world position is x = origin_x + ((float) i + u_x) * h: a
//     sum, a product, a sum.
//  4. Vertices are numbered by ascending cell id (k cy + j) cx + i.
//  5. A vertex carries the closest primitive at its position and that primitive's normal there: mdh_contacts' index and
//     normal at that point for the same kind list.
//  6. The grid edge along axis a from corner (i, j, k) emits a quad iff its a-coordinate is < cells[a], both other
//     coordinates lie in 1 .. cells - 1 (all four cells round the edge exist) and its endpoints differ in insideness.
//  7. With b = (a + 1) mod 3 and c = (a + 2) mod 3 the quad's vertices are those of the cells at (b, c) offsets (-1, -1),
//     (0, -1), (0, 0), (-1, 0) when the lower endpoint is inside -- the geometric normal then points along +a, out of the
//     solid -- and in the reverse order otherwise.
//  8. Quads are ordered by ascending key cornerid * 3 + a, cornerid = (k (cy + 1) + j) (cx + 1) + i.
//
// THE KERNELS.  No atomics anywhere: a vertex's and a quad's slot is a function of the grid alone.
//   k_surface_field, _listed   one lane per corner, a wavefront per 4 x 4 x 4 block of corners so that neighbours in space
//                              scan alike; sdf<PART> of the scene's variant, or the exact scan of the listed kinds
//   k_surface_count            a workgroup per 256 consecutive cell ids and the 256 corner ids of the same numbers: active
//                              cells and crossing edges by ballot and popcount, the workgroup's two totals through LDS
//   k_surface_scan             one workgroup: the exclusive scan of the workgroups' totals, in place; the totals are the
//                              counts the caller gets
//   k_surface_vertices, _listed  an active cell's slot is its workgroup's base + the wavefronts before it + mbcnt of the
//                              ballot; the lane writes the vertex, the cell-to-vertex map and, where asked, the arg-min
//                              (sdf_info<PART> or the listed scan) and its normal
//   k_surface_quads            the same addressing over the crossing edges, three flags a corner, reading the map
// Slots at or behind the caller's capacity are counted and not written.  The host has checked the grid (finite, inside
// +-1024, at most MDH_SURFACE_MAX_CORNERS corners: every id and 3 * id + 2 fit an int).
#pragma once

struct SurfaceArgs {
   float ox, oy, oz, h, iso;
   int cx, cy, cz;      // cells
   int vcap, qcap;      // the caller's capacities
   int nblocks;         // workgroups of k_surface_count: ceil (corners / MDH_BLOCK)
   float *field;        // scratch: the corners' values, x fastest
   int *map;            // scratch: a cell's vertex
   int *wg;             // scratch: [0, nblocks) the workgroups' vertices, [nblocks, 2 nblocks) their quads; bases behind the scan
   float *field_out;    // the caller's, any of them null
   float *positions, *normals;
   int *index, *quads;
   int *counts;         // [2]: vertices and quads found
};
MDH_DEV int surf_corners(const SurfaceArgs &a) { return (a.cx + 1) * (a.cy + 1) * (a.cz + 1); }
MDH_DEV int surf_cells(const SurfaceArgs &a) { return a.cx * a.cy * a.cz; }
MDH_DEV f3 surf_corner_point(const SurfaceArgs &a, int i, int j, int k)
{
   return F3(a.ox + (float)i * a.h, a.oy + (float)j * a.h, a.oz + (float)k * a.h);
}
// the corner of this lane in its wavefront's 4 x 4 x 4 block, or -1 (every thread has passed the kernel's barrier by then)
MDH_DEV int surf_field_corner(const SurfaceArgs &a, int &i, int &j, int &k)
{
   const int nx = a.cx + 1, ny = a.cy + 1, nz = a.cz + 1;
   const int bx = (nx + 3) >> 2, by = (ny + 3) >> 2, bz = (nz + 3) >> 2;
   const long w = (long)blockIdx.x * (MDH_BLOCK / 64) + (threadIdx.x >> 6);
   if (w >= (long)bx * by * bz) return -1;
   const int lane = threadIdx.x & 63, wi = (int)(w % bx), wj = (int)((w / bx) % by), wk = (int)(w / ((long)bx * by));
   i = wi * 4 + (lane & 3); j = wj * 4 + ((lane >> 2) & 3); k = wk * 4 + (lane >> 4);
   if (i >= nx || j >= ny || k >= nz) return -1;
   return (k * ny + j) * nx + i;
}
MDH_DEV void surf_field_store(const SurfaceArgs &a, int id, float v)
{
   a.field[id] = v;
   if (a.field_out) a.field_out[id] = v;
}
template <int PART> __global__ __launch_bounds__(MDH_BLOCK) void k_surface_field(KScene sc, SurfaceArgs a)
{
   static_assert(!(PART & (MDH_PF_CUSTOM | MDH_PF_POW2 | MDH_PF_ROOM | MDH_PF_PSMALL)), "the queries' variants: the general ones of built-in kinds");
   stage_table(sc); // (the kernel's only barrier: lanes without a corner leave behind it)
   int i, j, k;
   const int id = surf_field_corner(a, i, j, k);
   if (id < 0) return;
   surf_field_store(a, id, sdf<PART>(sc, surf_corner_point(a, i, j, k)) - a.iso);
}
template <bool GTAB> __global__ __launch_bounds__(MDH_BLOCK) void k_surface_field_listed(KScene sc, SurfaceArgs a, ListedArgs la)
{
   stage_table(sc);
   int i, j, k, index;
   const int id = surf_field_corner(a, i, j, k);
   if (id < 0) return;
   surf_field_store(a, id, listed_closest<GTAB>(sc, la, surf_corner_point(a, i, j, k), index) - a.iso);
}

// a cell's coordinates and its eight corner values -> its mask of inside corners (cell < surf_cells)
MDH_DEV int surf_cell_mask(const SurfaceArgs &a, int cell, int &i, int &j, int &k, float (&v)[8])
{
   const int nx = a.cx + 1, nxy = nx * (a.cy + 1);
   i = cell % a.cx; j = (cell / a.cx) % a.cy; k = cell / (a.cx * a.cy);
   const float *f = a.field + ((k * (a.cy + 1) + j) * nx + i);
   v[0] = f[0]; v[1] = f[1]; v[2] = f[nx]; v[3] = f[nx + 1];
   v[4] = f[nxy]; v[5] = f[nxy + 1]; v[6] = f[nxy + nx]; v[7] = f[nxy + nx + 1];
   int mask = 0;
#pragma unroll
   for (int c = 0; c < 8; ++c) mask |= (v[c] < 0.0f ? 1 : 0) << c;
   return mask;
}
MDH_DEV bool surf_active(int mask) { return mask != 0 && mask != 255; }
// a corner's three edges that emit a quad, bit a for axis a (corner < surf_corners); inside: the corner itself
MDH_DEV int surf_edge_flags(const SurfaceArgs &a, int corner, int &i, int &j, int &k, bool &inside)
{
   const int nx = a.cx + 1, ny = a.cy + 1;
   i = corner % nx; j = (corner / nx) % ny; k = corner / (nx * ny);
   const float *f = a.field + corner;
   inside = f[0] < 0.0f;
   const bool mi = i >= 1 && i < a.cx, mj = j >= 1 && j < a.cy, mk = k >= 1 && k < a.cz; // (strictly between the grid's faces)
   int flags = 0;
   if (i < a.cx && mj && mk && (f[1] < 0.0f) != inside) flags |= 1;
   if (j < a.cy && mk && mi && (f[nx] < 0.0f) != inside) flags |= 2;
   if (k < a.cz && mi && mj && (f[nx * ny] < 0.0f) != inside) flags |= 4;
   return flags;
}
MDH_DEV int surf_lanes_below(unsigned long long ballot)
{
   return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)ballot, 0u));
}
// what the wavefronts of this workgroup before this one counted (every thread of the workgroup calls it)
MDH_DEV int surf_waves_before(int *s_wave, int mine)
{
   const int wave = threadIdx.x >> 6;
   if ((threadIdx.x & 63) == 0) s_wave[wave] = mine;
   __syncthreads();
   int before = 0;
#pragma unroll
   for (int w = 0; w < MDH_BLOCK / 64; ++w) before += w < wave ? s_wave[w] : 0;
   return before;
}

__global__ __launch_bounds__(MDH_BLOCK) void k_surface_count(SurfaceArgs a)
{
   __shared__ int s_cells[MDH_BLOCK / 64], s_edges[MDH_BLOCK / 64];
   const int id = blockIdx.x * MDH_BLOCK + threadIdx.x; // (below nblocks * MDH_BLOCK < 2^24 + MDH_BLOCK)
   int i, j, k, flags = 0;
   bool active = false, inside;
   float v[8];
   if (id < surf_cells(a)) active = surf_active(surf_cell_mask(a, id, i, j, k, v));
   if (id < surf_corners(a)) flags = surf_edge_flags(a, id, i, j, k, inside);
   const int cells = __popcll(__ballot(active));
   const int edges = __popcll(__ballot(flags & 1)) + __popcll(__ballot(flags & 2)) + __popcll(__ballot(flags & 4));
   if ((threadIdx.x & 63) == 0) { s_cells[threadIdx.x >> 6] = cells; s_edges[threadIdx.x >> 6] = edges; }
   __syncthreads();
   if (threadIdx.x == 0) {
      int nc = 0, ne = 0;
      for (int w = 0; w < MDH_BLOCK / 64; ++w) { nc += s_cells[w]; ne += s_edges[w]; }
      a.wg[blockIdx.x] = nc;
      a.wg[a.nblocks + blockIdx.x] = ne;
   }
}

// one workgroup: both rows of a.wg become their exclusive scans, MDH_BLOCK entries a round with the carry of the rounds before
__global__ __launch_bounds__(MDH_BLOCK) void k_surface_scan(SurfaceArgs a)
{
   __shared__ int s_wave[MDH_BLOCK / 64];
   const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
   for (int row = 0; row < 2; ++row) {
      int *wg = a.wg + row * a.nblocks;
      int carry = 0;
      for (int base = 0; base < a.nblocks; base += MDH_BLOCK) { // (uniform: every thread runs every round)
         const int at = base + threadIdx.x;
         const int x = at < a.nblocks ? wg[at] : 0;
         int incl = x;
#pragma unroll
         for (int d = 1; d < 64; d <<= 1) {
            const int up = __shfl_up(incl, d, 64);
            if (lane >= d) incl += up;
         }
         if (lane == 63) s_wave[wave] = incl;
         __syncthreads();
         int before = 0, total = 0;
#pragma unroll
         for (int w = 0; w < MDH_BLOCK / 64; ++w) { before += w < wave ? s_wave[w] : 0; total += s_wave[w]; }
         if (at < a.nblocks) wg[at] = carry + before + incl - x;
         carry += total;
         __syncthreads(); // (s_wave is rewritten by the next round)
      }
      if (threadIdx.x == 0) a.counts[row] = carry;
   }
}

// one crossing test of step 3: axis A, edge E of the cell whose corner values are v
template <int A, int E> MDH_DEV void surf_edge(const float (&v)[8], float &sx, float &sy, float &sz, int &m)
{
   constexpr int o1 = E & 1, o2 = E >> 1;
   constexpr int c0 = A == 0 ? (o1 << 1 | o2 << 2) : A == 1 ? (o1 | o2 << 2) : (o1 | o2 << 1), c1 = c0 | (1 << A);
   const float v0 = v[c0], v1 = v[c1];
   if ((v0 < 0.0f) == (v1 < 0.0f)) return;
   const float t = v0 / (v0 - v1);
   sx = sx + (A == 0 ? t : (float)o1);
   sy = sy + (A == 1 ? t : (float)(A == 0 ? o1 : o2));
   sz = sz + (A == 2 ? t : (float)o2);
   ++m;
}
MDH_DEV f3 surf_vertex(const SurfaceArgs &a, int i, int j, int k, const float (&v)[8])
{
   float sx = 0.0f, sy = 0.0f, sz = 0.0f;
   int m = 0;
   surf_edge<0, 0>(v, sx, sy, sz, m); surf_edge<0, 1>(v, sx, sy, sz, m); surf_edge<0, 2>(v, sx, sy, sz, m); surf_edge<0, 3>(v, sx, sy, sz, m);
   surf_edge<1, 0>(v, sx, sy, sz, m); surf_edge<1, 1>(v, sx, sy, sz, m); surf_edge<1, 2>(v, sx, sy, sz, m); surf_edge<1, 3>(v, sx, sy, sz, m);
   surf_edge<2, 0>(v, sx, sy, sz, m); surf_edge<2, 1>(v, sx, sy, sz, m); surf_edge<2, 2>(v, sx, sy, sz, m); surf_edge<2, 3>(v, sx, sy, sz, m);
   const float fm = (float)m;
   return F3(a.ox + ((float)i + sx / fm) * a.h, a.oy + ((float)j + sy / fm) * a.h, a.oz + ((float)k + sz / fm) * a.h);
}
// the cell of this lane: its slot among the vertices, or -1 (not active); every thread of the workgroup comes through here
MDH_DEV int surf_vertex_slot(const SurfaceArgs &a, int *s_wave, int cell, int &i, int &j, int &k, float (&v)[8])
{
   bool active = false;
   if (cell < surf_cells(a)) active = surf_active(surf_cell_mask(a, cell, i, j, k, v));
   const unsigned long long ballot = __ballot(active);
   const int before = surf_waves_before(s_wave, __popcll(ballot));
   return active ? a.wg[blockIdx.x] + before + surf_lanes_below(ballot) : -1;
}
MDH_DEV void surf_vertex_store(const SurfaceArgs &a, int slot, int index, f3 N)
{
   if (a.index) a.index[slot] = index;
   if (a.normals) { a.normals[3 * slot] = N.x; a.normals[3 * slot + 1] = N.y; a.normals[3 * slot + 2] = N.z; }
}
template <int PART> __global__ __launch_bounds__(MDH_BLOCK) void k_surface_vertices(KScene sc, SurfaceArgs a)
{
   static_assert(!(PART & (MDH_PF_CUSTOM | MDH_PF_POW2 | MDH_PF_ROOM | MDH_PF_PSMALL)), "the queries' variants: the general ones of built-in kinds");
   __shared__ int s_wave[MDH_BLOCK / 64];
   stage_table(sc);
   int i, j, k;
   float v[8];
   const int cell = blockIdx.x * MDH_BLOCK + threadIdx.x;
   const int slot = surf_vertex_slot(a, s_wave, cell, i, j, k, v); // (the second and last barrier is in here)
   if (slot < 0) return;
   a.map[cell] = slot;
   if (slot >= a.vcap) return;
   const f3 x = surf_vertex(a, i, j, k, v);
   if (a.positions) { a.positions[3 * slot] = x.x; a.positions[3 * slot + 1] = x.y; a.positions[3 * slot + 2] = x.z; }
   if (!a.index && !a.normals) return;
   int index = -1, material;
   (void)sdf_info<PART>(sc, x, index);
   f3 N = F3(0.0f, 0.0f, 0.0f);
   if (a.normals && index >= 0) primitive_info<false, (PART & MDH_PF_GTAB) != 0>(sc, index, x, N, material);
   surf_vertex_store(a, slot, index, N);
}
template <bool GTAB> __global__ __launch_bounds__(MDH_BLOCK) void k_surface_vertices_listed(KScene sc, SurfaceArgs a, ListedArgs la)
{
   __shared__ int s_wave[MDH_BLOCK / 64];
   stage_table(sc);
   int i, j, k;
   float v[8];
   const int cell = blockIdx.x * MDH_BLOCK + threadIdx.x;
   const int slot = surf_vertex_slot(a, s_wave, cell, i, j, k, v);
   if (slot < 0) return;
   a.map[cell] = slot;
   if (slot >= a.vcap) return;
   const f3 x = surf_vertex(a, i, j, k, v);
   if (a.positions) { a.positions[3 * slot] = x.x; a.positions[3 * slot + 1] = x.y; a.positions[3 * slot + 2] = x.z; }
   if (!a.index && !a.normals) return;
   int index = -1, material;
   (void)listed_closest<GTAB>(sc, la, x, index);
   f3 N = F3(0.0f, 0.0f, 0.0f);
   if (a.normals && index >= 0) primitive_info<false, GTAB>(sc, index, x, N, material);
   surf_vertex_store(a, slot, index, N);
}

// the quad of the edge along A from corner (i, j, k): steps 6 and 7 (the four cells exist: surf_edge_flags)
template <int A> MDH_DEV void surf_quad_store(const SurfaceArgs &a, int slot, int i, int j, int k, bool inside)
{
   // the cell at offsets (ob, oc) along b = (A + 1) mod 3 and c = (A + 2) mod 3
   auto cell = [&](int ob, int oc) {
      const int ci = i + (A == 2 ? ob : A == 1 ? oc : 0), cj = j + (A == 0 ? ob : A == 2 ? oc : 0), ck = k + (A == 1 ? ob : A == 0 ? oc : 0);
      return a.map[(ck * a.cy + cj) * a.cx + ci];
   };
   const int q0 = cell(-1, -1), q1 = cell(0, -1), q2 = cell(0, 0), q3 = cell(-1, 0);
   int *out = a.quads + 4 * slot; // (four stores: the caller's array need not be aligned to a quad)
   out[0] = inside ? q0 : q3; out[1] = inside ? q1 : q2; out[2] = inside ? q2 : q1; out[3] = inside ? q3 : q0;
}
__global__ __launch_bounds__(MDH_BLOCK) void k_surface_quads(SurfaceArgs a)
{
   __shared__ int s_wave[MDH_BLOCK / 64];
   const int corner = blockIdx.x * MDH_BLOCK + threadIdx.x;
   int i, j, k, flags = 0;
   bool inside = false;
   if (corner < surf_corners(a)) flags = surf_edge_flags(a, corner, i, j, k, inside);
   const unsigned long long bx = __ballot(flags & 1), by = __ballot(flags & 2), bz = __ballot(flags & 4);
   const int before = surf_waves_before(s_wave, __popcll(bx) + __popcll(by) + __popcll(bz)); // (the kernel's only barrier)
   if (!flags) return;
   int slot = a.wg[a.nblocks + blockIdx.x] + before + surf_lanes_below(bx) + surf_lanes_below(by) + surf_lanes_below(bz);
   if ((flags & 1) && slot < a.qcap) surf_quad_store<0>(a, slot, i, j, k, inside);
   slot += flags & 1;
   if ((flags & 2) && slot < a.qcap) surf_quad_store<1>(a, slot, i, j, k, inside);
   slot += (flags >> 1) & 1;
   if ((flags & 4) && slot < a.qcap) surf_quad_store<2>(a, slot, i, j, k, inside);
}
