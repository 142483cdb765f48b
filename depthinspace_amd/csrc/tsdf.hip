// A track's per-frame disparity maps integrated into a truncated signed distance volume, and the volume turned into an indexed triangle
// mesh by naive surface nets (include/dis_hip.h, section "volumetric fusion"): fp32, every operation a fixed expression in the operand
// order of tests/tsdf_ref.py.  Order and hand-off between the launches are held by the launch boundaries alone - no atomics, no flags
// polled between workgroups - so nothing depends on where workgroups are placed and two calls give the same bits.
//
// One lane per lattice point, 256 consecutive points of the linear order (k, j, i) per block, so the lanes run along x and every dense
// load and store is coalesced; a block's points are a contiguous range of that order, which is also the order of the cells (cell
// (i, j, k) belongs to the lane of lattice point (i, j, k)), so block offset + rank inside the block is the rank in the whole volume.
//
//   tsdf_integrate_kernel  R, t and K are uniform and come through the scalar cache.  Every lattice point forms its own X from its
//                          indices (no incremental update along a row) and projects it into the tl frames; the tl disparities (and
//                          values) are asked for before any is used.  9 bytes stored per point.
//   tsdf_flag_kernel       stages the four rows of the block's eight-corner stencil in LDS - the linear ranges [b, b + 257) at the
//                          offsets 0, nx, nx ny and nx ny + nx, each a coalesced load, read 2 x from LDS - and writes one byte per
//                          lattice point: bit 0 the cell is active, bits 1 .. 3 the lattice edge along x, y, z crosses the surface
//                          and lies where a quad can exist, bit 4 tsdf < 0; and the block's count of active cells (64-bit ballots).
//   tsdf_quad_kernel       a crossing edge yields a quad when its four cells are active (their flag bytes; crossings are sparse):
//                          one byte of three quad bits per lattice point and the block's count of quads.
//   tsdf_scan_kernel       two workgroups of 1024 lanes, one per count array: exclusive offsets, the totals -> count[2].
//   tsdf_vertex_kernel     the dense vertex ids (rank or -1) of all cells; an active cell reads its eight corners again (active
//                          cells are a few per cent of the volume) and writes its vertex at its rank.
//   tsdf_face_kernel       a quad's two triangles at twice its rank, from the dense vertex ids.
#include "track_common.h"

#define TSDF_BLOCK TRACK_BLOCK
#define TSDF_MAX_TL TRACK_MAX_TL

struct TsdfParams {
  int tl, h, w, hw, nx, ny, nz, total;   // total = nx ny nz <= 2^30
  TrackCamera cam;
  float ox, oy, oz, voxel, trunc;
};

struct MeshParams {
  int nx, ny, nz, total, min_weight, vcap, fcap;
  float ox, oy, oz, voxel;
};

__global__ __launch_bounds__(TSDF_BLOCK) void tsdf_integrate_kernel(const float* __restrict__ disp, const float* __restrict__ R,
                                                                    const float* __restrict__ t, const float* __restrict__ value,
                                                                    float* __restrict__ tsdf_o, unsigned char* __restrict__ weight_o,
                                                                    float* __restrict__ vvalue_o, const TsdfParams p) {
  const int l = blockIdx.x * TSDF_BLOCK + threadIdx.x;
  if (l >= p.total) return;
  const int i = l % p.nx, r = l / p.nx;
  const int j = r % p.ny, k = r / p.ny;
  const float X[3] = {p.ox + (float)i * p.voxel, p.oy + (float)j * p.voxel, p.oz + (float)k * p.voxel};
  // first every projection and its gather, then the arithmetic
  float zf[TSDF_MAX_TL], df[TSDF_MAX_TL], vf[TSDF_MAX_TL];
  bool in[TSDF_MAX_TL];
#pragma unroll
  for (int f = 0; f < TSDF_MAX_TL; ++f) {
    in[f] = false;
    zf[f] = 0.f, df[f] = 0.f, vf[f] = 0.f;
    if (f < p.tl) {
      float Xc[3];
      track_to_camera(R + f * 9, t + f * 3, X, Xc);
      const bool front = Xc[2] > 0.f;
      const float zs = front ? Xc[2] : 1.f;
      // this projection is tsdf's own: fuse has (fx * X0) / X2 + cx, pose fx * (X0 * (1 / X2)) + cx, neither rounded
      const float pu = floorf((p.cam.fx * (Xc[0] / zs) + p.cam.cx) + 0.5f);
      const float pv = floorf((p.cam.fy * (Xc[1] / zs) + p.cam.cy) + 0.5f);
      // compared as floats before any conversion (every comparison is false for NaN)
      in[f] = front && pu >= 0.f && pu <= (float)(p.w - 1) && pv >= 0.f && pv <= (float)(p.h - 1);
      const int idx = in[f] ? f * p.hw + (int)pv * p.w + (int)pu : 0;   // < tl h w <= 2^28
      zf[f] = Xc[2];
      df[f] = disp[idx];
      vf[f] = value ? value[idx] : 0.f;
    }
  }
  float acc = 0.f, vsum = 0.f;
  int wt = 0, vc = 0;
#pragma unroll
  for (int f = 0; f < TSDF_MAX_TL; ++f) {
    if (!(in[f] && track_valid(df[f]))) continue;
    const float depth = p.cam.fb / df[f];
    const float sdf = depth - zf[f];
    if (sdf < -p.trunc) continue;   // behind the surface
    acc = acc + fminf(sdf / p.trunc, 1.f);
    ++wt;
    if (sdf <= p.trunc) {
      vsum = vsum + vf[f];
      ++vc;
    }
  }
  tsdf_o[l] = wt > 0 ? acc / (float)wt : 1.f;
  weight_o[l] = (unsigned char)wt;
  vvalue_o[l] = vc > 0 ? vsum / (float)vc : 0.f;
}

#define TSDF_F_ACTIVE 1
#define TSDF_F_NEG 16

__global__ __launch_bounds__(TSDF_BLOCK) void tsdf_flag_kernel(const float* __restrict__ tsdf, const unsigned char* __restrict__ weight,
                                                               unsigned char* __restrict__ flags, int* __restrict__ block_count,
                                                               const MeshParams p) {
  __shared__ float sf[4][TSDF_BLOCK + 4];
  __shared__ unsigned char sw[4][TSDF_BLOCK + 4];
  const int tid = threadIdx.x;
  const int b0 = blockIdx.x * TSDF_BLOCK;
  const int nxy = p.nx * p.ny;
  // rows dy + 2 dz of the stencil: 257 points each; a point past the end of the volume belongs to no cell's stencil (weight 0)
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int off = (s & 1) * p.nx + (s >> 1) * nxy;
    const long g = (long)b0 + off + tid;
    const bool ok = g < p.total;
    sf[s][tid] = ok ? tsdf[g] : 1.f;
    sw[s][tid] = ok ? weight[g] : 0;
  }
  if (tid < 4) {
    const int off = (tid & 1) * p.nx + (tid >> 1) * nxy;
    const long g = (long)b0 + off + TSDF_BLOCK;
    const bool ok = g < p.total;
    sf[tid][TSDF_BLOCK] = ok ? tsdf[g] : 1.f;
    sw[tid][TSDF_BLOCK] = ok ? weight[g] : 0;
  }
  __syncthreads();
  const int l = b0 + tid;
  bool active = false;
  if (l < p.total) {
    const int i = l % p.nx, r = l / p.nx;
    const int j = r % p.ny, k = r / p.ny;
    const bool xi = i <= p.nx - 2, yi = j <= p.ny - 2, zi = k <= p.nz - 2;        // the edge along the axis exists
    const bool xm = i >= 1 && xi, ym = j >= 1 && yi, zm = k >= 1 && zi;           // 1 <= index <= n - 2
    const bool neg0 = sf[0][tid] < 0.f;
    unsigned f = neg0 ? TSDF_F_NEG : 0;
    if (xi && yi && zi) {
      int nneg = 0;
      bool allok = true;
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const int s = ((c >> 1) & 1) + 2 * (c >> 2), e = tid + (c & 1);
        nneg += sf[s][e] < 0.f ? 1 : 0;
        allok = allok && (int)sw[s][e] >= p.min_weight;
      }
      active = allok && nneg > 0 && nneg < 8;
    }
    if (active) f |= TSDF_F_ACTIVE;
    if (xi && ym && zm && (sf[0][tid + 1] < 0.f) != neg0) f |= 2;
    if (yi && zm && xm && (sf[1][tid] < 0.f) != neg0) f |= 4;
    if (zi && xm && ym && (sf[2][tid] < 0.f) != neg0) f |= 8;
    flags[l] = (unsigned char)f;
  }
  track_block_count(__popcll(__ballot(active)), block_count);
}

// the quad bits of lattice point l = (i, j, k): bit a is set when the edge along axis a crosses and its four cells are active
__device__ __forceinline__ unsigned tsdf_quad_bits(const unsigned char* __restrict__ flags, unsigned f, int l, int nx, int nxy) {
  unsigned q = 0;
  // the cells (-1, -1), (0, -1), (0, 0), (-1, 0) along (a + 1, a + 2): strides (nx, nxy) for x, (nxy, 1) for y, (1, nx) for z
  if ((f & 2) && (flags[l - nx - nxy] & flags[l - nxy] & f & flags[l - nx] & TSDF_F_ACTIVE)) q |= 1;
  if ((f & 4) && (flags[l - nxy - 1] & flags[l - 1] & f & flags[l - nxy] & TSDF_F_ACTIVE)) q |= 2;
  if ((f & 8) && (flags[l - 1 - nx] & flags[l - nx] & f & flags[l - 1] & TSDF_F_ACTIVE)) q |= 4;
  return q;
}

__global__ __launch_bounds__(TSDF_BLOCK) void tsdf_quad_kernel(const unsigned char* __restrict__ flags, unsigned char* __restrict__ qmask,
                                                               int* __restrict__ block_count, const MeshParams p) {
  const int l = blockIdx.x * TSDF_BLOCK + threadIdx.x;
  unsigned q = 0;
  if (l < p.total) {
    const unsigned f = flags[l];
    if (f & 14) q = tsdf_quad_bits(flags, f, l, p.nx, p.nx * p.ny);   // (a crossing bit implies that the four cells exist)
    qmask[l] = (unsigned char)q;
  }
  track_block_count((__popcll(__ballot(q & 1)) + __popcll(__ballot(q & 2))) + __popcll(__ballot(q & 4)), block_count);
}

// workgroup s: exclusive scan of counts[s][0 .. nblocks) -> offs[s][0 .. nblocks], offs[s][nblocks] the total; count[s] = mul[s] * total
__global__ __launch_bounds__(TRACK_SCAN) void tsdf_scan_kernel(const int* __restrict__ vcount, const int* __restrict__ qcount, int* voff,
                                                               int* qoff, int* __restrict__ count, int nblocks) {
  const int total = track_scan(blockIdx.x == 0 ? vcount : qcount, blockIdx.x == 0 ? voff : qoff, nblocks);
  if (threadIdx.x == 0) count[blockIdx.x] = blockIdx.x == 0 ? total : 2 * total;   // two triangles per quad
}

__global__ __launch_bounds__(TSDF_BLOCK) void tsdf_vertex_kernel(const float* __restrict__ tsdf, const unsigned char* __restrict__ weight,
                                                                 const float* __restrict__ vvalue, const unsigned char* __restrict__ flags,
                                                                 const int* __restrict__ block_off, int* __restrict__ vid,
                                                                 float* __restrict__ xyz, float* __restrict__ normal,
                                                                 float* __restrict__ value, unsigned char* __restrict__ views,
                                                                 int* __restrict__ cell, const MeshParams p) {
  __shared__ int wave_count[TSDF_BLOCK / DIS_WAVE];
  const int l = blockIdx.x * TSDF_BLOCK + threadIdx.x;
  const bool inside = l < p.total;
  const bool active = inside && (flags[l] & TSDF_F_ACTIVE);
  const unsigned long long mask = __ballot(active);
  track_wave_counts(__popcll(mask), wave_count);
  if (!inside) return;
  const int i = l % p.nx, r = l / p.nx;
  const int j = r % p.ny, k = r / p.ny;
  if (i > p.nx - 2 || j > p.ny - 2 || k > p.nz - 2) return;   // no cell
  const size_t ci = ((size_t)k * (p.ny - 1) + j) * (p.nx - 1) + i;
  if (!active) {
    vid[ci] = -1;
    return;
  }
  const int rank = track_rank(block_off, wave_count, __popcll(mask & track_lanes_below()));
  vid[ci] = rank;
  if ((unsigned)rank >= (unsigned)p.vcap) return;
  const int nxy = p.nx * p.ny;
  float F[8], vs = 0.f;
  bool neg[8];
  int vw = 255;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const int g = l + (c & 1) + ((c >> 1) & 1) * p.nx + (c >> 2) * nxy;
    F[c] = tsdf[g];
    neg[c] = F[c] < 0.f;
    const float v = vvalue[g];
    vs = c == 0 ? v : vs + v;
    vw = min(vw, (int)weight[g]);
  }
  float sums[3] = {0.f, 0.f, 0.f}, g3[3] = {0.f, 0.f, 0.f};
  int cnt = 0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const int b = (a + 1) % 3, c_ = (a + 2) % 3;
#pragma unroll
    for (int pq = 0; pq < 4; ++pq) {
      const int pp = pq >> 1, qq = pq & 1;
      const int lo = (pp << b) | (qq << c_), hi = lo | (1 << a);
      const float fa = F[lo], fb = F[hi];
      if (neg[lo] != neg[hi]) {
        sums[a] = sums[a] + fa / (fa - fb);
        sums[b] = sums[b] + (float)pp;
        sums[c_] = sums[c_] + (float)qq;
        ++cnt;
      }
      const float d = fb - fa;
      g3[a] = pq == 0 ? d : g3[a] + d;
    }
  }
  const float nc = (float)cnt;   // >= 1: the corner signs differ, so an edge crosses
  const float len = sqrtf((g3[0] * g3[0] + g3[1] * g3[1]) + g3[2] * g3[2]);
  const bool okn = track_pos_finite(len);
  const size_t o = (size_t)rank * 3;
  xyz[o] = p.ox + ((float)i + sums[0] / nc) * p.voxel;
  xyz[o + 1] = p.oy + ((float)j + sums[1] / nc) * p.voxel;
  xyz[o + 2] = p.oz + ((float)k + sums[2] / nc) * p.voxel;
#pragma unroll
  for (int a = 0; a < 3; ++a) normal[o + a] = okn ? g3[a] / len : 0.f;
  value[rank] = vs / 8.f;
  views[rank] = (unsigned char)vw;
  cell[rank] = (int)ci;
}

__global__ __launch_bounds__(TSDF_BLOCK) void tsdf_face_kernel(const unsigned char* __restrict__ flags, const unsigned char* __restrict__ qmask,
                                                               const int* __restrict__ block_off, const int* __restrict__ vid,
                                                               int* __restrict__ faces, const MeshParams p) {
  __shared__ int wave_count[TSDF_BLOCK / DIS_WAVE];
  const int l = blockIdx.x * TSDF_BLOCK + threadIdx.x;
  const unsigned q = l < p.total ? qmask[l] : 0;
  const unsigned long long m0 = __ballot(q & 1), m1 = __ballot(q & 2), m2 = __ballot(q & 4);
  track_wave_counts((__popcll(m0) + __popcll(m1)) + __popcll(m2), wave_count);
  if (!q) return;
  const unsigned long long lower = track_lanes_below();
  int rank = track_rank(block_off, wave_count, (__popcll(m0 & lower) + __popcll(m1 & lower)) + __popcll(m2 & lower));
  const int i = l % p.nx, r = l / p.nx;
  const int j = r % p.ny, k = r / p.ny;
  const int cx = p.nx - 1, cy = p.ny - 1;
  const bool rev = !(flags[l] & TSDF_F_NEG);   // tsdf[p] >= 0
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    if (!(q & (1u << a))) continue;
    int v[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int ob = (s == 1 || s == 2) ? 0 : -1, oc = s >= 2 ? 0 : -1;   // (-1, -1), (0, -1), (0, 0), (-1, 0) along (a + 1, a + 2)
      int c[3] = {i, j, k};
      c[(a + 1) % 3] += ob;
      c[(a + 2) % 3] += oc;
      v[s] = vid[((size_t)c[2] * cy + c[1]) * cx + c[0]];
    }
    const int q0 = rev ? v[3] : v[0], q1 = rev ? v[2] : v[1], q2 = rev ? v[1] : v[2], q3 = rev ? v[0] : v[3];
    const int t0 = 2 * rank;
    // a triangle at or beyond fcap, or one that names a vertex at or beyond vcap, is counted but not written
    if ((unsigned)t0 < (unsigned)p.fcap && (unsigned)q0 < (unsigned)p.vcap && (unsigned)q1 < (unsigned)p.vcap &&
        (unsigned)q2 < (unsigned)p.vcap) {
      const size_t o = (size_t)t0 * 3;
      faces[o] = q0, faces[o + 1] = q1, faces[o + 2] = q2;
    }
    if ((unsigned)(t0 + 1) < (unsigned)p.fcap && (unsigned)q0 < (unsigned)p.vcap && (unsigned)q2 < (unsigned)p.vcap &&
        (unsigned)q3 < (unsigned)p.vcap) {
      const size_t o = (size_t)(t0 + 1) * 3;
      faces[o] = q0, faces[o + 1] = q2, faces[o + 2] = q3;
    }
    ++rank;
  }
}

extern "C" int dis_tsdf_integrate(const float* disp, const float* R, const float* t, const float* K4_host, float baseline, const float* value,
                                  const float* origin3_host, float voxel, float trunc, float* tsdf, unsigned char* weight, float* vvalue,
                                  int tl, int h, int w, int nx, int ny, int nz, void* stream) {
  if (!disp || !R || !t || !K4_host || !origin3_host || !tsdf || !weight || !vvalue) return DIS_ERR_NULL;
  if (tl < 1 || tl > TSDF_MAX_TL || !track_image_ok(h, w, 2) || !tsdf_grid_ok(nx, ny, nz)) return DIS_ERR_BAD_SHAPE;
  TsdfParams p;
  if (!track_pos_finite(voxel) || !track_pos_finite(trunc) || !track_camera(K4_host, baseline, &p.cam) ||
      !tsdf_origin(origin3_host, &p.ox, &p.oy, &p.oz))
    return DIS_ERR_UNSUPPORTED;
  p.tl = tl, p.h = h, p.w = w, p.hw = h * w, p.nx = nx, p.ny = ny, p.nz = nz, p.total = nx * ny * nz;
  p.voxel = voxel, p.trunc = trunc;
  hipLaunchKernelGGL(tsdf_integrate_kernel, dim3((unsigned)dis_cdiv(p.total, TSDF_BLOCK)), dim3(TSDF_BLOCK), 0, (hipStream_t)stream, disp, R, t,
                     value, tsdf, weight, vvalue, p);
  DIS_CHECK_LAUNCH();
  return 0;
}

struct TsdfMeshPlan {
  long total, cells, nblocks;
  long off_flags, off_qmask, off_vcount, off_qcount, off_voff, off_qoff, off_vid, bytes;   // byte offsets inside the workspace
};

// false: unsupported extents
static bool tsdf_mesh_plan(int nx, int ny, int nz, TsdfMeshPlan* pl) {
  if (!tsdf_grid_ok(nx, ny, nz)) return false;
  pl->total = (long)nx * ny * nz;
  pl->cells = (long)(nx - 1) * (ny - 1) * (nz - 1);
  pl->nblocks = (pl->total + TSDF_BLOCK - 1) / TSDF_BLOCK;
  TrackCarver ws = {16, 0};
  pl->off_flags = ws.take(pl->total);
  pl->off_qmask = ws.take(pl->total);
  pl->off_vcount = ws.take(pl->nblocks * 4);
  pl->off_qcount = ws.take(pl->nblocks * 4);
  pl->off_voff = ws.take((pl->nblocks + 1) * 4);
  pl->off_qoff = ws.take((pl->nblocks + 1) * 4);
  pl->off_vid = ws.take(pl->cells * 4);
  pl->bytes = ws.off;
  return true;
}

extern "C" long dis_tsdf_mesh_workspace(int nx, int ny, int nz) {
  TsdfMeshPlan pl;
  if (!tsdf_mesh_plan(nx, ny, nz, &pl)) return -1;
  return pl.bytes;
}

extern "C" int dis_tsdf_mesh(const float* tsdf, const unsigned char* weight, const float* vvalue, const float* origin3_host, float voxel,
                             int min_weight, int vcap, int fcap, const DisTsdfMeshOut* out, int nx, int ny, int nz, void* workspace,
                             long workspace_bytes, void* stream) {
  if (!tsdf || !weight || !vvalue || !origin3_host || !out || !workspace) return DIS_ERR_NULL;
  if (!out->count) return DIS_ERR_NULL;
  if (vcap > 0 && (!out->xyz || !out->normal || !out->value || !out->views || !out->cell)) return DIS_ERR_NULL;
  if (fcap > 0 && !out->faces) return DIS_ERR_NULL;
  TsdfMeshPlan pl;
  if (!tsdf_mesh_plan(nx, ny, nz, &pl)) return DIS_ERR_BAD_SHAPE;
  MeshParams p;
  if (!track_pos_finite(voxel) || !tsdf_origin(origin3_host, &p.ox, &p.oy, &p.oz) || min_weight < 1 || min_weight > TSDF_MAX_TL ||
      vcap < 0 || fcap < 0 || workspace_bytes < pl.bytes || ((uintptr_t)workspace & 15))
    return DIS_ERR_UNSUPPORTED;
  p.nx = nx, p.ny = ny, p.nz = nz, p.total = (int)pl.total, p.min_weight = min_weight, p.vcap = vcap, p.fcap = fcap, p.voxel = voxel;
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  unsigned char* flags = (unsigned char*)(ws + pl.off_flags);
  unsigned char* qmask = (unsigned char*)(ws + pl.off_qmask);
  int* vcount = (int*)(ws + pl.off_vcount);
  int* qcount = (int*)(ws + pl.off_qcount);
  int* voff = (int*)(ws + pl.off_voff);
  int* qoff = (int*)(ws + pl.off_qoff);
  int* vid = out->vid ? out->vid : (int*)(ws + pl.off_vid);
  const dim3 grid((unsigned)pl.nblocks), block(TSDF_BLOCK);
  hipLaunchKernelGGL(tsdf_flag_kernel, grid, block, 0, st, tsdf, weight, flags, vcount, p);
  DIS_CHECK_LAUNCH();
  hipLaunchKernelGGL(tsdf_quad_kernel, grid, block, 0, st, (const unsigned char*)flags, qmask, qcount, p);
  DIS_CHECK_LAUNCH();
  hipLaunchKernelGGL(tsdf_scan_kernel, dim3(2), dim3(TRACK_SCAN), 0, st, (const int*)vcount, (const int*)qcount, voff, qoff, out->count,
                     (int)pl.nblocks);
  DIS_CHECK_LAUNCH();
  hipLaunchKernelGGL(tsdf_vertex_kernel, grid, block, 0, st, tsdf, weight, vvalue, (const unsigned char*)flags, (const int*)voff, vid, out->xyz,
                     out->normal, out->value, out->views, out->cell, p);
  DIS_CHECK_LAUNCH();
  hipLaunchKernelGGL(tsdf_face_kernel, grid, block, 0, st, (const unsigned char*)flags, (const unsigned char*)qmask, (const int*)qoff,
                     (const int*)vid, out->faces, p);
  DIS_CHECK_LAUNCH();
  return 0;
}
