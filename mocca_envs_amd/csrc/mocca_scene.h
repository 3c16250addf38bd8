// mocca_scene.h -- what the ray caster (mocca_render.hip) and the depth camera (mocca_depth.hip) share of one env's scene: the kinematics
// walk that gives every link its frame, the robot's geoms (or its skeleton) as world-space primitives, and the ray / sphere, ray / tube
// and ray / height-field intersections.  (Planks, boxes, cylinders and the height of a cell: mocca_rays.h, shared with the height scan
// too.)  Device code only; one definition, two users.
#pragma once
#include "mocca_rays.h"

namespace mocca_rdr {

constexpr int MAX_PRIMS = MOCCA_MAX_GEOMS + 1;         // the robot's geoms and the walk target
constexpr int PRIM_WORDS = 12;                         // p1 (3), radius, p2 (3), id, colour (3), kind
constexpr float SKELETON_RADIUS = 0.04f;               // of the link capsules a model without drawable geoms is shown by

DI void matmul3(const float* A, const float* B, float* C) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) C[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
}
DI void matvec3(const float* A, const float* v, float* o) {
#pragma unroll
  for (int i = 0; i < 3; ++i) o[i] = A[3 * i] * v[0] + A[3 * i + 1] * v[1] + A[3 * i + 2] * v[2];
}

// The kinematics walk: per body R (9, row-major, world <- body), origin in world (3), COM in world (3) into fr[b * 15 ..], for the
// bodies 0 .. nb - 1 (nb <= M->n_bodies: parent[b] < b, so the first nb bodies hold all their own ancestors, and a body's frame comes out
// the same whatever nb is).  `fr` is global memory (link_frames_kernel: the thread reads back its own stores) or LDS.
DI void walk_frames(const MoccaModel* M, const float* st, float* fr, int nb) {
  const float x = st[3], y = st[4], z = st[5], w = st[6];
  const float pos[3] = {st[0], st[1], st[2]};
  fr[0] = 1 - 2 * (y * y + z * z); fr[1] = 2 * (x * y - z * w); fr[2] = 2 * (x * z + y * w);
  fr[3] = 2 * (x * y + z * w); fr[4] = 1 - 2 * (x * x + z * z); fr[5] = 2 * (y * z - x * w);
  fr[6] = 2 * (x * z - y * w); fr[7] = 2 * (y * z + x * w); fr[8] = 1 - 2 * (x * x + y * y);
  fr[9] = 0.0f; fr[10] = 0.0f; fr[11] = 0.0f;   // origins relative to the base until the last pass, as the oracle keeps them
#pragma unroll 1
  for (int b = 1; b < nb; ++b) {
    const int p = M->parent[b];
    float Rp[9], rp[3], jr[9], ax[3], jp[3], Rq[9], T[9], R[9], off[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) { Rp[k] = fr[15 * p + k]; jr[k] = M->jrot[b][k]; }
#pragma unroll
    for (int k = 0; k < 3; ++k) { rp[k] = fr[15 * p + 9 + k]; ax[k] = M->jaxis[b][k]; jp[k] = M->jpos[b][k]; }
    const float th = st[MOCCA_STATE_BASE + b - 1];
    const float c = cosf(th), s = sinf(th), t = 1 - c;
    Rq[0] = c + t * ax[0] * ax[0];         Rq[1] = t * ax[0] * ax[1] - s * ax[2]; Rq[2] = t * ax[0] * ax[2] + s * ax[1];
    Rq[3] = t * ax[0] * ax[1] + s * ax[2]; Rq[4] = c + t * ax[1] * ax[1];         Rq[5] = t * ax[1] * ax[2] - s * ax[0];
    Rq[6] = t * ax[0] * ax[2] - s * ax[1]; Rq[7] = t * ax[1] * ax[2] + s * ax[0]; Rq[8] = c + t * ax[2] * ax[2];
    matmul3(Rp, jr, T);
    matmul3(T, Rq, R);
    matvec3(Rp, jp, off);
#pragma unroll
    for (int k = 0; k < 9; ++k) fr[15 * b + k] = R[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) fr[15 * b + 9 + k] = rp[k] + off[k];
  }
#pragma unroll 1
  for (int b = 0; b < nb; ++b) {
    float R[9], cw[3];
    const float cl[3] = {M->com[b][0], M->com[b][1], M->com[b][2]};
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = fr[15 * b + k];
    matvec3(R, cl, cw);
#pragma unroll
    for (int k = 0; k < 3; ++k) {   // the base position is added last: world = (relative sum) + pos
      const float rel = fr[15 * b + 9 + k];
      fr[15 * b + 12 + k] = (rel + cw[k]) + pos[k];
      fr[15 * b + 9 + k] = rel + pos[k];
    }
  }
}

// The robot as primitives: lane g of one wave turns geom g into a world-space record out[g * PRIM_WORDS ..] from the frames `fr` of
// walk_frames (all n_bodies of them); a model whose geoms are all points: its skeleton.  Words 8 .. 10, the base colour palette[body & 7],
// are written only where `palette` is given.  Every lane of the wave calls this; the number of records comes back, wave-uniform.
DI int stage_robot(const MoccaModel* M, const float* fr, int lane, float* out, const float (*palette)[3]) {
  const int ng = M->n_geoms > MOCCA_MAX_GEOMS ? MOCCA_MAX_GEOMS : M->n_geoms;
  const int nb = M->n_bodies > MOCCA_MAX_BODIES ? MOCCA_MAX_BODIES : M->n_bodies;
  // A model whose geoms are all points (radius 0: Cassie's links are meshes in the reference, and the blob keeps only their hull support
  // points) has nothing a ray can hit: it is drawn as its skeleton instead, see below.  Wave-uniform.
  const bool skeleton = __ballot(lane < ng && M->g_radius[lane < ng ? lane : 0] > 0.0f) == 0ull;
  int nrobot = ng;
  if (!skeleton) {
    if (lane < ng) {
      int b = M->g_body[lane];
      b = b < 0 ? 0 : (b > nb - 1 ? nb - 1 : b);
      float p1[3], p2[3];
      const float l1[3] = {M->g_p1[lane][0], M->g_p1[lane][1], M->g_p1[lane][2]}, l2[3] = {M->g_p2[lane][0], M->g_p2[lane][1], M->g_p2[lane][2]};
      matvec3(fr + 15 * b, l1, p1);
      matvec3(fr + 15 * b, l2, p2);
      float* o = out + lane * PRIM_WORDS;
#pragma unroll
      for (int k = 0; k < 3; ++k) { o[k] = p1[k] + fr[15 * b + 9 + k]; o[4 + k] = p2[k] + fr[15 * b + 9 + k]; }
      if (palette) {
#pragma unroll
        for (int k = 0; k < 3; ++k) o[8 + k] = palette[b & 7][k];
      }
      o[3] = M->g_radius[lane];
      o[7] = __int_as_float(lane);
      o[11] = __int_as_float(M->g_type[lane] == MOCCA_GEOM_CAPSULE ? 1 : 0);
    }
  } else {
    // The skeleton: for every body b >= 1 a capsule of radius SKELETON_RADIUS from its parent's origin to its own (slot b - 1), and for
    // every body without children one from its origin through its centre of mass to twice that distance (toes, Cassie's rods), in the
    // slots after them; ids MOCCA_RENDER_ID_LINK0 + b.  At most MAX_PRIMS - 1 records: leaves beyond that are not drawn.
    const bool body = lane >= 1 && lane < nb;
    bool leaf = body;
    for (int c = 1; c < nb; ++c) leaf = leaf && M->parent[c] != lane;
    const unsigned long long leaves = __ballot(leaf);
    const int slot = (nb - 1) + __popcll(leaves & ((1ull << lane) - 1ull));
    nrobot = (nb - 1) + __popcll(leaves);
    nrobot = nrobot > MAX_PRIMS - 1 ? MAX_PRIMS - 1 : nrobot;
    if (body) {
      int p = M->parent[lane];
      p = p < 0 ? 0 : (p > nb - 1 ? nb - 1 : p);
      float* o = out + (lane - 1) * PRIM_WORDS;
#pragma unroll
      for (int k = 0; k < 3; ++k) { o[k] = fr[15 * p + 9 + k]; o[4 + k] = fr[15 * lane + 9 + k]; }
      if (palette) {
#pragma unroll
        for (int k = 0; k < 3; ++k) o[8 + k] = palette[lane & 7][k];
      }
      o[3] = SKELETON_RADIUS; o[7] = __int_as_float(MOCCA_RENDER_ID_LINK0 + lane); o[11] = __int_as_float(1);
    }
    if (leaf && slot < MAX_PRIMS - 1) {
      float* o = out + slot * PRIM_WORDS;
#pragma unroll
      for (int k = 0; k < 3; ++k) { o[k] = fr[15 * lane + 9 + k]; o[4 + k] = 2.0f * fr[15 * lane + 12 + k] - fr[15 * lane + 9 + k]; }
      if (palette) {
#pragma unroll
        for (int k = 0; k < 3; ++k) o[8 + k] = palette[lane & 7][k];
      }
      o[3] = SKELETON_RADIUS; o[7] = __int_as_float(MOCCA_RENDER_ID_LINK0 + lane); o[11] = __int_as_float(1);
    }
  }
  return nrobot;
}

// ---- ray / primitive intersections.  The ray is o + t d with d . forward = 1: t IS the depth along the view axis.  Each returns the entry
// parameter (the ray starts outside), or a negative number for a miss. ----
DI float hit_sphere(const float* o, const float* d, float dd, const float* c, float r) {
  const float oc[3] = {o[0] - c[0], o[1] - c[1], o[2] - c[2]};
  const float b = oc[0] * d[0] + oc[1] * d[1] + oc[2] * d[2];
  const float cc = oc[0] * oc[0] + oc[1] * oc[1] + oc[2] * oc[2] - r * r;
  const float h = b * b - dd * cc;
  if (h < 0.0f) return -1.0f;
  return (-b - sqrtf(h)) / dd;
}
// lateral surface of the cylinder of radius r around the segment pa pb, between its ends
DI float hit_tube(const float* o, const float* d, float dd, const float* pa, const float* pb, float r) {
  const float ba[3] = {pb[0] - pa[0], pb[1] - pa[1], pb[2] - pa[2]}, oa[3] = {o[0] - pa[0], o[1] - pa[1], o[2] - pa[2]};
  const float baba = ba[0] * ba[0] + ba[1] * ba[1] + ba[2] * ba[2];
  const float bard = ba[0] * d[0] + ba[1] * d[1] + ba[2] * d[2], baoa = ba[0] * oa[0] + ba[1] * oa[1] + ba[2] * oa[2];
  const float rdoa = d[0] * oa[0] + d[1] * oa[1] + d[2] * oa[2], oaoa = oa[0] * oa[0] + oa[1] * oa[1] + oa[2] * oa[2];
  const float A = baba * dd - bard * bard, B = baba * rdoa - baoa * bard, C = baba * oaoa - baoa * baoa - r * r * baba;
  if (!(A > 1e-12f * baba * dd)) return -1.0f;   // the ray runs along the axis: it can only enter through an end sphere
  const float h = B * B - A * C;
  if (h < 0.0f) return -1.0f;
  const float t = (-B - sqrtf(h)) / A;
  const float yy = baoa + t * bard;
  return (yy > 0.0f && yy < baba) ? t : -1.0f;
}
// (hit_box, hit_cylinder and cell_height: mocca_rays.h, shared with the height scan)

// The height-field march.  The surface is a height function, so along the ray g(t) = z(t) - height(x(t), y(t)) is continuous and piecewise
// linear, with a kink where the ray crosses a cell border or a cell's diagonal; the first sign change of g is the hit.  The march walks
// the cells under the ray (a 2-D DDA), samples g at each cell's entry, diagonal crossing and exit, and interpolates inside the piece whose
// ends differ in sign: no ray slips between two triangles.  Trip count: a ray crosses at most (cols - 1) + (rows - 1) + 1 cells.
DI float hit_heightfield(const HeightField hf, const float* o, const float* d, float tnear, float tfar, float* nrm) {
  const float sc = hf.scale, hx = 0.5f * (float)(hf.cols - 1), hy = 0.5f * (float)(hf.rows - 1);
  const float ox = o[0] * sc + hx, oy = o[1] * sc + hy, dx = d[0] * sc, dy = d[1] * sc;   // grid coordinates: vertex (i, j) at (i, j)
  float ta = tnear, tb = tfar;
  // clip to the grid's box [0, cols - 1] x [0, rows - 1] x [zmin, zmax]
  const float zpad = 1e-3f * (hf.zmax - hf.zmin) + 1e-4f;   // the march starts strictly above the highest vertex
  const float lo3[3] = {0.0f, 0.0f, hf.zmin - zpad}, hi3[3] = {(float)(hf.cols - 1), (float)(hf.rows - 1), hf.zmax + zpad};
  const float o3[3] = {ox, oy, o[2]}, d3[3] = {dx, dy, d[2]};
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    if (fabsf(d3[k]) < 1e-20f) {
      if (o3[k] < lo3[k] || o3[k] > hi3[k]) return -1.0f;
    } else {
      const float inv = 1.0f / d3[k];
      float t0 = (lo3[k] - o3[k]) * inv, t1 = (hi3[k] - o3[k]) * inv;
      if (t0 > t1) { const float s = t0; t0 = t1; t1 = s; }
      ta = fmaxf(ta, t0); tb = fminf(tb, t1);
    }
  }
  if (!(ta <= tb)) return -1.0f;
  const int ci = hf.cols - 2, cj = hf.rows - 2;
  const float tmid0 = ta + 1e-4f * (tb - ta);   // the first cell is the one just inside the entry point
  int i = (int)floorf(ox + tmid0 * dx), j = (int)floorf(oy + tmid0 * dy);
  i = i < 0 ? 0 : (i > ci ? ci : i);
  j = j < 0 ? 0 : (j > cj ? cj : j);
  const int si = dx > 0.0f ? 1 : -1, sj = dy > 0.0f ? 1 : -1;
  const float idx = fabsf(dx) > 1e-20f ? 1.0f / dx : 0.0f, idy = fabsf(dy) > 1e-20f ? 1.0f / dy : 0.0f;
  float t0 = ta, gprev = 0.0f;
  bool have = false;
  const int max_cells = hf.cols + hf.rows - 1;   // (cols - 1) + (rows - 1) + 1
#pragma unroll 1
  for (int step = 0; step < max_cells; ++step) {
    // where the ray leaves cell (i, j)
    const float tx = idx != 0.0f ? ((float)(dx > 0.0f ? i + 1 : i) - ox) * idx : 1e30f;
    const float ty = idy != 0.0f ? ((float)(dy > 0.0f ? j + 1 : j) - oy) * idy : 1e30f;
    float t1 = fminf(fminf(tx, ty), tb);
    t1 = fmaxf(t1, t0);
    const float* row = hf.data + (size_t)j * hf.cols + i;
    const float h00 = row[0], h10 = row[1], h01 = row[hf.cols], h11 = row[hf.cols + 1];
    const float z0 = o[2] + t0 * d[2], z1 = o[2] + t1 * d[2];
    const float top = fmaxf(fmaxf(h00, h10), fmaxf(h01, h11));
    if (have && gprev > 0.0f && fminf(z0, z1) > top) {
      gprev = z1 - top;   // above this whole cell: g stays positive
    } else {
      const float u0 = ox + t0 * dx - (float)i, v0 = oy + t0 * dy - (float)j, u1 = ox + t1 * dx - (float)i, v1 = oy + t1 * dy - (float)j;
      const float s0 = u0 + v0, s1 = u1 + v1;
      float tk[3], gk[3];
      int nk = 0;
      tk[nk] = t0; gk[nk++] = z0 - cell_height(h00, h10, h01, h11, u0, v0);
      if ((s0 < 1.0f) != (s1 < 1.0f) && s0 != s1) {   // the diagonal lies between entry and exit
        float tm = t0 + (1.0f - s0) / (s1 - s0) * (t1 - t0);
        tm = fminf(fmaxf(tm, t0), t1);
        const float um = ox + tm * dx - (float)i, vm = oy + tm * dy - (float)j;
        tk[nk] = tm; gk[nk++] = o[2] + tm * d[2] - (h00 + um * (h10 - h00) + vm * (h01 - h00));
      }
      tk[nk] = t1; gk[nk++] = z1 - cell_height(h00, h10, h01, h11, u1, v1);
      float tp = t0, gp = have ? gprev : gk[0];
      have = true;
      for (int k = 0; k < nk; ++k) {
        if ((gp > 0.0f) != (gk[k] > 0.0f)) {
          const float den = gp - gk[k];
          const float th = den != 0.0f ? tp + gp / den * (tk[k] - tp) : tp;
          // the triangle under the hit point
          const float uh = ox + th * dx - (float)i, vh = oy + th * dy - (float)j;
          const float gx = uh + vh <= 1.0f ? (h10 - h00) : (h11 - h01), gy = uh + vh <= 1.0f ? (h01 - h00) : (h11 - h10);
          const float nx = -gx * sc, ny = -gy * sc, il = 1.0f / sqrtf(nx * nx + ny * ny + 1.0f);
          nrm[0] = nx * il; nrm[1] = ny * il; nrm[2] = il;
          return th;
        }
        tp = tk[k]; gp = gk[k];
      }
      gprev = gp;
    }
    if (t1 >= tb) break;
    if (tx <= ty) i += si; else j += sj;
    if (i < 0 || i > ci || j < 0 || j > cj) break;
    t0 = t1;
  }
  return -1.0f;
}

// What a ray meets first.  S: n_prims records of PRIM_WORDS (the robot, and for the ray caster the walk target), PL: n_planks plank frames;
// the ray is o + t d.  Returns the depth of the nearest surface entered in [tnear, tfar), tfar where there is none.  DETAIL (the ray
// caster): also the id, the primitive's index (or -1) and the surface normal, into *h.  Without DETAIL (the depth camera, on the training
// path) h is not touched, and a ray that is not finite is kept out of the height-field march.  Robot and plank loops have wave-uniform trip
// counts and every lane reads the same record (an LDS broadcast); the height-field march is the only divergent loop.
struct RayHit { int id, bestk; float nrm[3]; };
template <bool DETAIL>
DI float nearest_hit(const float* S, int n_prims, const float* PL, int n_planks, bool cylinder, const float* ph, bool ground, const HeightField& hf,
                     const float* o, const float* d, float tnear, float tfar, RayHit* h) {
  const float dd = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
  float best = tfar;
  int id = MOCCA_RENDER_ID_NONE, bestk = -1, sub = 0;
  float nrm[3] = {0.0f, 0.0f, 1.0f};
#pragma unroll 1
  for (int k = 0; k < n_prims; ++k) {
    const float* P = S + k * PRIM_WORDS;
    const float pa[3] = {P[0], P[1], P[2]}, pb[3] = {P[4], P[5], P[6]};
    const float r = P[3];
    float t = hit_sphere(o, d, dd, pa, r);
    int part = 0;
    if (__float_as_int(P[11]) != 0) {   // capsule: the nearest of its two end spheres and the tube between them
      const float t2 = hit_sphere(o, d, dd, pb, r), t3 = hit_tube(o, d, dd, pa, pb, r);
      if (t2 >= 0.0f && (t < 0.0f || t2 < t)) { t = t2; part = 1; }
      if (t3 >= 0.0f && (t < 0.0f || t3 < t)) { t = t3; part = 2; }
    }
    // (a geom of radius 0 -- a hull support point -- is nothing a ray can enter, though rounding can make its discriminant >= 0)
    if (r > 0.0f && t >= tnear && t < best) { best = t; bestk = k; sub = part; }
  }
  if (DETAIL && bestk >= 0) {
    const float* P = S + bestk * PRIM_WORDS;
    id = __float_as_int(P[7]);
    const float hp[3] = {o[0] + best * d[0], o[1] + best * d[1], o[2] + best * d[2]};
    float c[3] = {P[0], P[1], P[2]};
    if (sub == 1) { c[0] = P[4]; c[1] = P[5]; c[2] = P[6]; }
    if (sub == 2) {   // foot of the hit point on the axis
      const float ba[3] = {P[4] - P[0], P[5] - P[1], P[6] - P[2]};
      const float s = ((hp[0] - P[0]) * ba[0] + (hp[1] - P[1]) * ba[1] + (hp[2] - P[2]) * ba[2]) / (ba[0] * ba[0] + ba[1] * ba[1] + ba[2] * ba[2]);
#pragma unroll
      for (int k = 0; k < 3; ++k) c[k] = P[k] + s * ba[k];
    }
    const float ir = 1.0f / P[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) nrm[k] = (hp[k] - c[k]) * ir;
  }
  // the live planks
#pragma unroll 1
  for (int k = 0; k < n_planks; ++k) {
    const float* B = PL + k * PLANK_WORDS;
    const float rel[3] = {o[0] - B[9], o[1] - B[10], o[2] - B[11]};
    float lo[3], ld[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {   // into the plank frame: R^T
      lo[a] = B[a] * rel[0] + B[3 + a] * rel[1] + B[6 + a] * rel[2];
      ld[a] = B[a] * d[0] + B[3 + a] * d[1] + B[6 + a] * d[2];
    }
    int part = 0;
    const float t = cylinder ? hit_cylinder(lo, ld, ph, &part) : hit_box(lo, ld, ph, &part);
    if (t >= tnear && t < best) {
      best = t; bestk = -1; id = MOCCA_RENDER_ID_PLANK0 + k;
      if (DETAIL) {
        float ln[3] = {0.0f, 0.0f, 0.0f};
        if (cylinder) {
          if (part == 1) ln[2] = ld[2] < 0.0f ? 1.0f : -1.0f;
          else { const float ir = 1.0f / ph[0]; ln[0] = (lo[0] + t * ld[0]) * ir; ln[1] = (lo[1] + t * ld[1]) * ir; }
        } else {
          ln[part] = ld[part] < 0.0f ? 1.0f : -1.0f;
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) nrm[a] = B[3 * a] * ln[0] + B[3 * a + 1] * ln[1] + B[3 * a + 2] * ln[2];
      }
    }
  }
  // the ground plane z = 0 of the tasks that keep it
  if (ground && d[2] < 0.0f && o[2] > 0.0f) {
    const float t = -o[2] / d[2];
    if (t >= tnear && t < best) { best = t; bestk = -1; id = MOCCA_RENDER_ID_GROUND; nrm[0] = 0.0f; nrm[1] = 0.0f; nrm[2] = 1.0f; }
  }
  // the planner envs' terrain
  if (hf.data && (DETAIL || (fabsf(dd) < 1e30f && fabsf(o[0]) < 1e30f && fabsf(o[1]) < 1e30f && fabsf(o[2]) < 1e30f))) {
    float hn[3];
    const float t = hit_heightfield(hf, o, d, tnear, best, hn);
    if (t >= tnear && t < best) { best = t; bestk = -1; id = MOCCA_RENDER_ID_HEIGHTFIELD; nrm[0] = hn[0]; nrm[1] = hn[1]; nrm[2] = hn[2]; }
  }
  if (DETAIL) {
    h->id = id; h->bestk = bestk;
    h->nrm[0] = nrm[0]; h->nrm[1] = nrm[1]; h->nrm[2] = nrm[2];
  }
  return best;
}

}  // namespace mocca_rdr
