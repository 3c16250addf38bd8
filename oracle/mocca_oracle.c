/*
 * mocca_oracle.c -- CPU restatement of the vectorised locomotion stepper.
 *
 * TEST INFRASTRUCTURE ONLY.  Nothing under mocca_envs_amd/ may import, link or
 * call this file; it is the checker for the HIP path (tests/, bench.py's
 * cpu_baseline leg, __graft_entry__.smoke()).
 *
 * PARITY STATUS
 *   task / observation / reward arithmetic : pinned against golden vectors
 *       captured by importing the reference (tests/golden/, tools/make_golden.py).
 *   rigid-body physics                     : *** parity unpinned ***.  The
 *       reference's physics lives in the third-party `pybullet` wheel
 *       (un-pinned in /root/reference/setup.py:11), which is neither vendored
 *       nor installable here and for which the reference holds no golden
 *       vectors.  This file restates the published algorithms Bullet's
 *       btMultiBodyDynamicsWorld is built from -- Featherstone's articulated
 *       body algorithm, projected Gauss-Seidel over contact / friction /
 *       joint-limit rows with Baumgarte (ERP) stabilisation, symplectic Euler --
 *       at the call sites the reference drives them from:
 *         setJointMotorControlArray(TORQUE_CONTROL) robots.py:35-40
 *         stepSimulation()                          bullet_utils.py:352-353
 *         physics parameters                        bullet_utils.py:340-350, env_base.py:78-83
 *       and checks them with physical invariants (tests/test_oracle_physics.py).
 *
 * Build: compiled twice by oracle/Makefile, -DREAL=float (what the GPU must
 * match) and -DREAL=double (the reference arithmetic width).
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "mocca_model.h"

#ifndef REAL
#define REAL double
#endif
typedef REAL real;

#define MB MOCCA_MAX_BODIES
#define NDOF_MAX (6 + MB)
#define MAX_CONTACTS 24 /* storage; the live caps are MoccaModel.max_contacts / max_rows (<= 20 / 64: the HIP accuracy instance's) */
#define MAX_ROWS 64
#define DBG_WORDS 20    /* MOCCA_DEBUG_WORDS of include/mocca.h */
/* the HIP solver's lane layout (mocca_device.h MAXR): friction rows of contact i sit on lanes 46 - 2i, 47 - 2i -- 62 - 2i, 63 - 2i in the
 * 64-row instance, which runs the blobs whose caps exceed 48 rows / 12 contacts */
#define KERNEL_MAXR(m) (((m)->max_rows > 48 || (m)->max_contacts > 12) ? 64 : 48)

#if defined(__GNUC__)
#define API __attribute__((visibility("default")))
#else
#define API
#endif

/* ------------------------------------------------------------------ */
/* small linear algebra                                                */
/* ------------------------------------------------------------------ */
static inline real dot3(const real *a, const real *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
static inline void cross3(const real *a, const real *b, real *o) {
  real x = a[1] * b[2] - a[2] * b[1], y = a[2] * b[0] - a[0] * b[2], z = a[0] * b[1] - a[1] * b[0];
  o[0] = x; o[1] = y; o[2] = z;
}
static inline real dot6(const real *a, const real *b) {
  return a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3] + a[4] * b[4] + a[5] * b[5];
}
static inline void matvec3(const real *R, const real *x, real *o) {
  real a = R[0] * x[0] + R[1] * x[1] + R[2] * x[2];
  real b = R[3] * x[0] + R[4] * x[1] + R[5] * x[2];
  real c = R[6] * x[0] + R[7] * x[1] + R[8] * x[2];
  o[0] = a; o[1] = b; o[2] = c;
}
static inline void matmul3(const real *A, const real *B, real *C) {
  real T[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) T[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
  memcpy(C, T, sizeof(T));
}
static void quat_to_mat(const real *q, real *R) { /* q = (x,y,z,w) */
  real x = q[0], y = q[1], z = q[2], w = q[3];
  R[0] = 1 - 2 * (y * y + z * z); R[1] = 2 * (x * y - z * w); R[2] = 2 * (x * z + y * w);
  R[3] = 2 * (x * y + z * w); R[4] = 1 - 2 * (x * x + z * z); R[5] = 2 * (y * z - x * w);
  R[6] = 2 * (x * z - y * w); R[7] = 2 * (y * z + x * w); R[8] = 1 - 2 * (x * x + y * y);
}
/* rotation about unit axis a by angle th (Rodrigues) */
static void axis_angle_mat(const real *a, real th, real *R) {
  real c = cos(th), s = sin(th), t = 1 - c;
  R[0] = c + t * a[0] * a[0];        R[1] = t * a[0] * a[1] - s * a[2]; R[2] = t * a[0] * a[2] + s * a[1];
  R[3] = t * a[0] * a[1] + s * a[2]; R[4] = c + t * a[1] * a[1];        R[5] = t * a[1] * a[2] - s * a[0];
  R[6] = t * a[0] * a[2] - s * a[1]; R[7] = t * a[1] * a[2] + s * a[0]; R[8] = c + t * a[2] * a[2];
}
/* spatial motion cross  v x m  (ang;lin) */
static inline void crm(const real *v, const real *m, real *o) {
  real a[3], b[3], c[3];
  cross3(v, m, a);
  cross3(v, m + 3, b);
  cross3(v + 3, m, c);
  o[0] = a[0]; o[1] = a[1]; o[2] = a[2];
  o[3] = b[0] + c[0]; o[4] = b[1] + c[1]; o[5] = b[2] + c[2];
}
/* spatial force cross  v x* f */
static inline void crf(const real *v, const real *f, real *o) {
  real a[3], b[3], c[3];
  cross3(v, f, a);
  cross3(v + 3, f + 3, b);
  cross3(v, f + 3, c);
  o[0] = a[0] + b[0]; o[1] = a[1] + b[1]; o[2] = a[2] + b[2];
  o[3] = c[0]; o[4] = c[1]; o[5] = c[2];
}
/* Cholesky inverse of a symmetric positive definite 6x6 (row-major full storage) */
static void spd6_inverse(const real *A, real *Ainv) {
  real L[36];
  memset(L, 0, sizeof(L));
  for (int j = 0; j < 6; ++j) {
    real s = A[6 * j + j];
    for (int k = 0; k < j; ++k) s -= L[6 * j + k] * L[6 * j + k];
    real d = sqrt(s);
    L[6 * j + j] = d;
    real id = 1 / d;
    for (int i = j + 1; i < 6; ++i) {
      real t = A[6 * i + j];
      for (int k = 0; k < j; ++k) t -= L[6 * i + k] * L[6 * j + k];
      L[6 * i + j] = t * id;
    }
  }
  /* invert L (lower) */
  real Li[36];
  memset(Li, 0, sizeof(Li));
  for (int j = 0; j < 6; ++j) {
    Li[6 * j + j] = 1 / L[6 * j + j];
    for (int i = j + 1; i < 6; ++i) {
      real t = 0;
      for (int k = j; k < i; ++k) t -= L[6 * i + k] * Li[6 * k + j];
      Li[6 * i + j] = t / L[6 * i + i];
    }
  }
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < 6; ++j) {
      real t = 0;
      for (int k = (i > j ? i : j); k < 6; ++k) t += Li[6 * k + i] * Li[6 * k + j];
      Ainv[6 * i + j] = t;
    }
}

/* ------------------------------------------------------------------ */
/* Philox4x32-10, keyed (seed), counter (block, episode, env, stream)  */
/* ------------------------------------------------------------------ */
static void philox4x32(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t *out) {
  for (int r = 0; r < 10; ++r) {
    uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
    uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
/* d-th uniform in [0,1) of (seed, env, episode): 24-bit mantissa so f32 and f64 agree exactly */
static real rng_uniform(uint64_t seed, uint32_t env, uint32_t episode, uint32_t d) {
  uint32_t o[4];
  philox4x32(d >> 2, episode, env, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), o);
  return (real)((o[d & 3] >> 8) * (1.0f / 16777216.0f));
}

/* ------------------------------------------------------------------ */
/* environment storage                                                 */
/* ------------------------------------------------------------------ */
typedef struct {
  real pos[3], quat[4], vel[3], omg[3];
  real q[MB], qd[MB]; /* index = body, [0] unused */
  real warm[MOCCA_MAX_SLOTS];
} Dyn;

typedef struct {
  real walk_target[3];
  real linear_potential, angular_potential;
  int32_t close_count;
  real stop_frames;
  int32_t done, t, episode, draw, mirrored;
  real feet_contact[MOCCA_MAX_FEET];
  real dist, angle;
  int32_t next_step_index, target_reached_count, stop_on_next_step, set_stop_on_next_step, curriculum;
  real applied_gain;
  real prev_body_x;
  /* Cassie (env_cassie.py:433-479) */
  real jvel[MOCCA_MAX_CTRL];
  real initial_z;
  int32_t istep;
  /* Stepper with random_reward (env_locomotion.py:533-547): this step's eight U(0.8, 1.2) weights */
  real rw[8];
  /* Stepper: which planks' covers each foot touched in the last step, bit 4 f + k (foot f, live plank k): what reset() reads stale (MOCCA_TASKF_STALE_RESET_CONTACTS) */
  int32_t cover;
} Task;

typedef struct {
  real terrain[MOCCA_MAX_TERRAIN_STEPS][6];        /* x y z phi x_tilt y_tilt, env_locomotion.py:441 */
  int32_t plank_info[MOCCA_MAX_PLANKS];            /* terrain row currently shown by plank k */
} Terrain;

/* per-substep workspace (kept so tests can inspect it) */
typedef struct {
  real R[MB][9], r[MB][3], a[MB][3]; /* body orientation, origin rel. base origin, hinge axis (world) */
  real S[MB][6], v[MB][6], c[MB][6], I[MB][36], pA[MB][6], IA[MB][36];
  real U[MB][6], d[MB], u[MB], acc[MB][6], qdd[MB];
  real IA0inv[36];
  real comw[MB][3]; /* link COM rel. base origin */
  /* contacts */
  int nc;
  int c_a[MAX_CONTACTS], c_b[MAX_CONTACTS], c_slot[MAX_CONTACTS];
  real c_P[MAX_CONTACTS][3], c_n[MAX_CONTACTS][3], c_depth[MAX_CONTACTS], c_mu[MAX_CONTACTS];
  real c_erp[MAX_CONTACTS], c_cfm[MAX_CONTACTS];
  int foot_touch[MOCCA_MAX_FEET];        /* any terrain contact of foot k this substep */
  int foot_target[MOCCA_MAX_FEET];       /* foot k touches the cover of the target plank */
  int cover;                             /* bit 4 f + k: foot f touches the cover of live plank k */
  int body_touch;                        /* some non-foot geom touches the terrain */
  /* rows */
  int nr;
  real J[MAX_ROWS][NDOF_MAX], Mi[MAX_ROWS][NDOF_MAX], A[MAX_ROWS][MAX_ROWS];
  real lam[MAX_ROWS], bias[MAX_ROWS], cfm[MAX_ROWS], w[MAX_ROWS];
  int row_kind[MAX_ROWS]; /* 0 limit, 1 normal, 2 friction, 3 closure */
  int row_normal[MAX_ROWS]; /* friction: index of its normal row */
  real row_mu[MAX_ROWS];
  int row_slot[MAX_ROWS];
  /* active set of the last substep, same words as the HIP path's debug record (include/mocca.h MOCCA_DBG_*) */
  int32_t dbg[DBG_WORDS]; /* words 12..15: THIS substep's cap flags / count / wanted rows, accumulated per env by dbg_commit() */
  int nc_wanted;          /* contacts within the margin before the max_contacts cap */
  /* MoccaModel.precise_gaps: body frames in double precision whatever `real` is, for the POSITION-level gaps of the constraint rows only */
  double Rd[MB][9], rd[MB][3];
  int precise; /* 0 off; bit 0 closure gaps, bit 1 flat-ground contact depth, bit 2 planar rows */
} Work;

typedef struct {
  MoccaModel m;
  int task_id, n_envs;
  uint64_t seed;
  int auto_reset, eval_mode, random_pose, random_reward;
  Dyn *dyn;
  Task *task;
  Terrain *ter;
  Work wk;
  int32_t *dbg; /* [n_envs][DBG_WORDS]: words 0..11 of wk.dbg after each env's last substep, words 12..15 accumulated (orc_clear_debug) */
  real feet_xyz[MOCCA_MAX_FEET][3];
  real body_rpy[3], body_vel[3];
  /* optional uniform tape: when set, every random draw pops from it instead of Philox, so the golden
   * tests can feed the oracle the very numbers a scripted numpy RandomState gave the reference */
  const double *tape;
  int tape_n, tape_pos;
  /* Cassie mocap / phase envs: the reference motion (orc_set_trajectory), [traj_n][MOCCA_TRAJ_STRIDE] */
  float *traj;
  int traj_n;
  double traj_tmax, traj_cstep;
  /* planner envs: the height field (orc_set_heightfield), data[iy * cols + ix], `hf_scale` grid points per metre */
  float *hf;
  int hf_rows, hf_cols;
  double hf_scale;
} Oracle;

static real draw_uniform(Oracle *o, int env, Task *tk) {
  if (o->tape) {
    real u = o->tape_pos < o->tape_n ? (real)o->tape[o->tape_pos] : (real)0.5;
    o->tape_pos++;
    tk->draw++;
    return u;
  }
  return rng_uniform(o->seed, (uint32_t)env, (uint32_t)tk->episode, (uint32_t)tk->draw++);
}

#define NJ(o) ((o)->m.n_joints)

/* ------------------------------------------------------------------ */
/* kinematics + ABA                                                    */
/* ------------------------------------------------------------------ */
static void kinematics(const MoccaModel *m, const Dyn *s, Work *w) {
  quat_to_mat(s->quat, w->R[0]);
  w->r[0][0] = w->r[0][1] = w->r[0][2] = 0;
  for (int b = 1; b < m->n_bodies; ++b) {
    int p = m->parent[b];
    real jr[9], ax[3], jp[3], Rq[9], T[9];
    for (int k = 0; k < 9; ++k) jr[k] = m->jrot[b][k];
    for (int k = 0; k < 3; ++k) { ax[k] = m->jaxis[b][k]; jp[k] = m->jpos[b][k]; }
    axis_angle_mat(ax, s->q[b], Rq);
    matmul3(w->R[p], jr, T);
    matvec3(T, ax, w->a[b]);
    matmul3(T, Rq, w->R[b]);
    real off[3];
    matvec3(w->R[p], jp, off);
    for (int k = 0; k < 3; ++k) w->r[b][k] = w->r[p][k] + off[k];
  }
  for (int b = 0; b < m->n_bodies; ++b) {
    real cl[3] = {m->com[b][0], m->com[b][1], m->com[b][2]}, cw[3];
    matvec3(w->R[b], cl, cw);
    for (int k = 0; k < 3; ++k) w->comw[b][k] = w->r[b][k] + cw[k];
  }
}

/* The same walk in double precision (experiment: orc_set_precise_gaps).  A constraint row's bias is (position gap) x erp / dt: the gap is a
 * difference of two ~1 m chains, fp32 leaves ~1e-7 m of rounding in it, and Cassie's dt = 0.6 ms turns that into 1e-4 m/s of velocity. */
static void kinematics_d(const MoccaModel *m, const Dyn *s, Work *w) {
  double x = s->quat[0], y = s->quat[1], z = s->quat[2], q = s->quat[3];
  double *R0 = w->Rd[0];
  R0[0] = 1 - 2 * (y * y + z * z); R0[1] = 2 * (x * y - z * q); R0[2] = 2 * (x * z + y * q);
  R0[3] = 2 * (x * y + z * q); R0[4] = 1 - 2 * (x * x + z * z); R0[5] = 2 * (y * z - x * q);
  R0[6] = 2 * (x * z - y * q); R0[7] = 2 * (y * z + x * q); R0[8] = 1 - 2 * (x * x + y * y);
  w->rd[0][0] = w->rd[0][1] = w->rd[0][2] = 0;
  for (int b = 1; b < m->n_bodies; ++b) {
    int p = m->parent[b];
    double a[3] = {m->jaxis[b][0], m->jaxis[b][1], m->jaxis[b][2]}, th = s->q[b], c = cos(th), sn = sin(th), t = 1 - c, Rq[9], T[9];
    Rq[0] = c + t * a[0] * a[0];         Rq[1] = t * a[0] * a[1] - sn * a[2]; Rq[2] = t * a[0] * a[2] + sn * a[1];
    Rq[3] = t * a[0] * a[1] + sn * a[2]; Rq[4] = c + t * a[1] * a[1];         Rq[5] = t * a[1] * a[2] - sn * a[0];
    Rq[6] = t * a[0] * a[2] - sn * a[1]; Rq[7] = t * a[1] * a[2] + sn * a[0]; Rq[8] = c + t * a[2] * a[2];
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) T[3 * i + j] = w->Rd[p][3 * i] * m->jrot[b][j] + w->Rd[p][3 * i + 1] * m->jrot[b][3 + j] + w->Rd[p][3 * i + 2] * m->jrot[b][6 + j];
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) w->Rd[b][3 * i + j] = T[3 * i] * Rq[j] + T[3 * i + 1] * Rq[3 + j] + T[3 * i + 2] * Rq[6 + j];
    for (int k = 0; k < 3; ++k)
      w->rd[b][k] = w->rd[p][k] + w->Rd[p][3 * k] * m->jpos[b][0] + w->Rd[p][3 * k + 1] * m->jpos[b][1] + w->Rd[p][3 * k + 2] * m->jpos[b][2];
  }
}

/* spatial inertia about the base origin, world axes */
static void body_inertia(const MoccaModel *m, const Work *w, int b, real *I) {
  real Il[9] = {m->inertia[b][0], m->inertia[b][3], m->inertia[b][4],
                m->inertia[b][3], m->inertia[b][1], m->inertia[b][5],
                m->inertia[b][4], m->inertia[b][5], m->inertia[b][2]};
  real T[9], Rt[9], Iw[9];
  const real *R = w->R[b];
  matmul3(R, Il, T);
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) Rt[3 * i + j] = R[3 * j + i];
  matmul3(T, Rt, Iw);
  real ms = m->mass[b];
  const real *c = w->comw[b];
  real cc = dot3(c, c);
  memset(I, 0, 36 * sizeof(real));
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) I[6 * i + j] = Iw[3 * i + j] + ms * ((i == j ? cc : 0) - c[i] * c[j]);
  /* m c^x upper-right, its transpose lower-left */
  real cx[9] = {0, -c[2], c[1], c[2], 0, -c[0], -c[1], c[0], 0};
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      I[6 * i + 3 + j] = ms * cx[3 * i + j];
      I[6 * (3 + i) + j] = ms * cx[3 * j + i];
    }
  for (int i = 0; i < 3; ++i) I[6 * (3 + i) + 3 + i] = ms;
}

static void matvec6(const real *M, const real *x, real *o) {
  real t[6];
  for (int i = 0; i < 6; ++i) t[i] = dot6(M + 6 * i, x);
  memcpy(o, t, sizeof(t));
}

/* Featherstone ABA about the (instantaneous) base origin in world axes.
 * tau[b] : generalised force on hinge b.  Outputs w->qdd, w->acc[0] (spatial). */
static void aba(const MoccaModel *m, const Dyn *s, const real *tau, Work *w, int with_bias) {
  int nb = m->n_bodies;
  /* pass 1 */
  for (int k = 0; k < 3; ++k) { w->v[0][k] = s->omg[k]; w->v[0][3 + k] = s->vel[k]; }
  for (int b = 1; b < nb; ++b) {
    int p = m->parent[b];
    real ra[3];
    cross3(w->r[b], w->a[b], ra);
    for (int k = 0; k < 3; ++k) { w->S[b][k] = w->a[b][k]; w->S[b][3 + k] = ra[k]; }
    real vJ[6];
    for (int k = 0; k < 6; ++k) vJ[k] = w->S[b][k] * s->qd[b];
    crm(w->v[p], vJ, w->c[b]);
    for (int k = 0; k < 6; ++k) w->v[b][k] = w->v[p][k] + vJ[k];
  }
  for (int b = 0; b < nb; ++b) {
    body_inertia(m, w, b, w->I[b]);
    memcpy(w->IA[b], w->I[b], 36 * sizeof(real));
    real Iv[6];
    matvec6(w->I[b], w->v[b], Iv);
    if (with_bias) crf(w->v[b], Iv, w->pA[b]);
    else memset(w->pA[b], 0, 6 * sizeof(real));
    if (!with_bias) { memset(w->c[b], 0, 6 * sizeof(real)); }
    /* gravity as an external force through the COM */
    if (with_bias) {
      real f[3] = {0, 0, -(real)m->gravity * (real)m->mass[b]}, n[3];
      cross3(w->comw[b], f, n);
      for (int k = 0; k < 3; ++k) { w->pA[b][k] -= n[k]; w->pA[b][3 + k] -= f[k]; }
    }
  }
  if (with_bias) {
    /* Link damping of btMultiBody (computeAccelerationsArticulatedBodyAlgorithmMultiDof, "adding damping terms (only)"): the base AND
     * every link carry a drag force  m v (k1 + k2 |v|)  through their COM (v = the COM's velocity) and a torque  Ic w (k1 + k2 |w|),
     * with k1 = k2 = m_linearDamping (resp. m_angularDamping), both 0.04 by default.  Restated from the published source as recalled;
     * [UNVERIFIED-BULLET] until a dump pins it.  (Rounds 1-3 early: base only, k1 only, force through the base origin.) */
    for (int b = 0; b < nb; ++b) {
      real ms = (real)m->mass[b];
      real Il[9] = {m->inertia[b][0], m->inertia[b][3], m->inertia[b][4],
                    m->inertia[b][3], m->inertia[b][1], m->inertia[b][5],
                    m->inertia[b][4], m->inertia[b][5], m->inertia[b][2]};
      real T[9], Rt[9], Iw[9], Iom[3], wxc[3], vc[3], F[3], tq[3], cxF[3];
      matmul3(w->R[b], Il, T);
      for (int i = 0; i < 3; ++i)
        for (int jj = 0; jj < 3; ++jj) Rt[3 * i + jj] = w->R[b][3 * jj + i];
      matmul3(T, Rt, Iw);
      const real *om = w->v[b];
      matvec3(Iw, om, Iom);
      cross3(om, w->comw[b], wxc);
      for (int k = 0; k < 3; ++k) vc[k] = w->v[b][3 + k] + wxc[k];
      real kl = (real)m->lin_damp * (1 + (real)sqrt(dot3(vc, vc))), ka = (real)m->ang_damp * (1 + (real)sqrt(dot3(om, om)));
      for (int k = 0; k < 3; ++k) { F[k] = kl * ms * vc[k]; tq[k] = ka * Iom[k]; }
      cross3(w->comw[b], F, cxF);
      for (int k = 0; k < 3; ++k) {
        w->pA[b][k] += tq[k] + cxF[k];
        w->pA[b][3 + k] += F[k];
      }
    }
  }
  /* pass 2 */
  for (int b = nb - 1; b >= 1; --b) {
    int p = m->parent[b];
    matvec6(w->IA[b], w->S[b], w->U[b]);
    w->d[b] = dot6(w->S[b], w->U[b]) + (real)m->jarm[b];
    real tq = tau[b] - (with_bias ? (real)m->jdamp[b] * s->qd[b] : 0);
    w->u[b] = tq - dot6(w->S[b], w->pA[b]);
    real id = 1 / w->d[b];
    real Ia[36], pa[6], Iac[6];
    for (int i = 0; i < 6; ++i)
      for (int j = 0; j < 6; ++j) Ia[6 * i + j] = w->IA[b][6 * i + j] - w->U[b][i] * w->U[b][j] * id;
    matvec6(Ia, w->c[b], Iac);
    for (int i = 0; i < 6; ++i) pa[i] = w->pA[b][i] + Iac[i] + w->U[b][i] * (w->u[b] * id);
    for (int i = 0; i < 36; ++i) w->IA[p][i] += Ia[i];
    for (int i = 0; i < 6; ++i) w->pA[p][i] += pa[i];
  }
  spd6_inverse(w->IA[0], w->IA0inv);
  real a0[6];
  matvec6(w->IA0inv, w->pA[0], a0);
  for (int k = 0; k < 6; ++k) w->acc[0][k] = -a0[k];
  /* pass 3 */
  for (int b = 1; b < nb; ++b) {
    int p = m->parent[b];
    real ap[6];
    for (int k = 0; k < 6; ++k) ap[k] = w->acc[p][k] + w->c[b][k];
    w->qdd[b] = (w->u[b] - dot6(w->U[b], ap)) / w->d[b];
    for (int k = 0; k < 6; ++k) w->acc[b][k] = ap[k] + w->S[b][k] * w->qdd[b];
  }
}

/* generalised acceleration response to a generalised force f (6 base + joints by body index at 5+b),
 * using the articulated quantities cached by the last aba() call: out = M^-1 f. */
static void minv_apply(const MoccaModel *m, const Work *w, const real *f, real *out) {
  int nb = m->n_bodies;
  real p[MB][6], uu[MB], a[MB][6];
  memset(p, 0, sizeof(p));
  for (int b = nb - 1; b >= 1; --b) {
    int pr = m->parent[b];
    uu[b] = f[5 + b] - dot6(w->S[b], p[b]);
    real s = uu[b] / w->d[b];
    for (int k = 0; k < 6; ++k) p[pr][k] += p[b][k] + w->U[b][k] * s;
  }
  real rhs[6];
  for (int k = 0; k < 6; ++k) rhs[k] = f[k] - p[0][k];
  matvec6(w->IA0inv, rhs, a[0]);
  for (int k = 0; k < 6; ++k) out[k] = a[0][k];
  for (int b = 1; b < nb; ++b) {
    int pr = m->parent[b];
    real qdd = (uu[b] - dot6(w->U[b], a[pr])) / w->d[b];
    out[5 + b] = qdd;
    for (int k = 0; k < 6; ++k) a[b][k] = a[pr][k] + w->S[b][k] * qdd;
  }
}

/* ------------------------------------------------------------------ */
/* collision detection                                                 */
/* ------------------------------------------------------------------ */
static void plane_space(const real *n, real *t1, real *t2) { /* btPlaneSpace1 */
  if (fabs(n[2]) > (real)0.7071067811865475244) {
    real a = n[1] * n[1] + n[2] * n[2], k = 1 / sqrt(a);
    t1[0] = 0; t1[1] = -n[2] * k; t1[2] = n[1] * k;
    t2[0] = a * k; t2[1] = -n[0] * t1[2]; t2[2] = n[0] * t1[1];
  } else {
    real a = n[0] * n[0] + n[1] * n[1], k = 1 / sqrt(a);
    t1[0] = -n[1] * k; t1[1] = n[0] * k; t1[2] = 0;
    t2[0] = -n[2] * t1[1]; t2[1] = n[2] * t1[0]; t2[2] = a * k;
  }
}

/* getQuaternionFromEuler (roll,pitch,yaw) -> rotation matrix Rz(yaw) Ry(pitch) Rx(roll) */
static void euler_to_mat(real roll, real pitch, real yaw, real *R) {
  real cr = cos(roll), sr = sin(roll), cp = cos(pitch), sp = sin(pitch), cy = cos(yaw), sy = sin(yaw);
  R[0] = cy * cp; R[1] = cy * sp * sr - sy * cr; R[2] = cy * sp * cr + sy * sr;
  R[3] = sy * cp; R[4] = sy * sp * sr + cy * cr; R[5] = sy * sp * cr - cy * sr;
  R[6] = -sp;     R[7] = cp * sr;                R[8] = cp * cr;
}

/* sphere (world centre C, radius rad) against a box with centre bc, rotation Rb (world<-box), half
 * extents h.  Returns gap (negative = penetration), normal n (box -> sphere), surface point on sphere. */
static real sphere_box(const real *C, real rad, const real *bc, const real *Rb, const real *h, real *n) {
  real d[3] = {C[0] - bc[0], C[1] - bc[1], C[2] - bc[2]}, l[3], q[3];
  for (int i = 0; i < 3; ++i) l[i] = Rb[i] * d[0] + Rb[3 + i] * d[1] + Rb[6 + i] * d[2]; /* Rb^T d */
  int inside = 1;
  for (int i = 0; i < 3; ++i) {
    q[i] = l[i];
    if (q[i] > h[i]) { q[i] = h[i]; inside = 0; }
    if (q[i] < -h[i]) { q[i] = -h[i]; inside = 0; }
  }
  real nl[3] = {0, 0, 0}, dist;
  if (!inside) {
    real e[3] = {l[0] - q[0], l[1] - q[1], l[2] - q[2]};
    dist = sqrt(dot3(e, e));
    for (int i = 0; i < 3; ++i) nl[i] = e[i] / dist;
  } else {
    /* centre inside the box: leave through the nearest face */
    int best = 0;
    real bd = h[0] - fabs(l[0]);
    for (int i = 1; i < 3; ++i) {
      real di = h[i] - fabs(l[i]);
      if (di < bd) { bd = di; best = i; }
    }
    nl[best] = l[best] >= 0 ? 1 : -1;
    dist = -bd;
  }
  matvec3(Rb, nl, n);
  return dist - rad;
}

/* the same against an upright cylinder (Pillar, bullet_objects.py:86-89): axis = local z, h = (radius, radius, half height) */
static real sphere_cylinder(const real *C, real rad, const real *bc, const real *Rb, const real *h, real *n) {
  real d[3] = {C[0] - bc[0], C[1] - bc[1], C[2] - bc[2]}, l[3];
  for (int i = 0; i < 3; ++i) l[i] = Rb[i] * d[0] + Rb[3 + i] * d[1] + Rb[6 + i] * d[2];
  real rho = sqrt(l[0] * l[0] + l[1] * l[1]), R = h[0], hz = h[2];
  real ux = rho > (real)1e-12 ? l[0] / rho : 1, uy = rho > (real)1e-12 ? l[1] / rho : 0; /* radial direction */
  real nl[3] = {0, 0, 0}, dist;
  if (rho <= R && fabs(l[2]) <= hz) { /* centre inside: leave through the nearer of cap / side */
    real dcap = hz - fabs(l[2]), dside = R - rho;
    if (dcap < dside) { nl[2] = l[2] >= 0 ? 1 : -1; dist = -dcap; }
    else { nl[0] = ux; nl[1] = uy; dist = -dside; }
  } else {
    real qr = rho < R ? rho : R, qz = l[2] > hz ? hz : (l[2] < -hz ? -hz : l[2]);
    real e[3] = {l[0] - qr * ux, l[1] - qr * uy, l[2] - qz};
    dist = sqrt(dot3(e, e));
    for (int i = 0; i < 3; ++i) nl[i] = e[i] / dist;
  }
  matvec3(Rb, nl, n);
  return dist - rad;
}

static void geom_point(const MoccaModel *m, const Work *w, int g, int e, real *C) {
  int b = m->g_body[g];
  real pl[3], pw[3];
  for (int k = 0; k < 3; ++k) pl[k] = e ? m->g_p2[g][k] : m->g_p1[g][k];
  matvec3(w->R[b], pl, pw);
  for (int k = 0; k < 3; ++k) C[k] = w->r[b][k] + pw[k];
}

/* closest points between segments p1-q1 and p2-q2 (Ericson, Real-Time Collision Detection 5.1.9) */
static void seg_seg(const real *p1, const real *q1, const real *p2, const real *q2, real *c1, real *c2) {
  real d1[3], d2[3], r[3];
  for (int k = 0; k < 3; ++k) { d1[k] = q1[k] - p1[k]; d2[k] = q2[k] - p2[k]; r[k] = p1[k] - p2[k]; }
  real a = dot3(d1, d1), e = dot3(d2, d2), f = dot3(d2, r), s, t;
  const real EPS = (real)1e-12;
  if (a <= EPS && e <= EPS) { s = t = 0; }
  else if (a <= EPS) { s = 0; t = f / e; t = t < 0 ? 0 : (t > 1 ? 1 : t); }
  else {
    real c = dot3(d1, r);
    if (e <= EPS) { t = 0; s = -c / a; s = s < 0 ? 0 : (s > 1 ? 1 : s); }
    else {
      real b = dot3(d1, d2), den = a * e - b * b;
      if (den > EPS) { s = (b * f - c * e) / den; s = s < 0 ? 0 : (s > 1 ? 1 : s); }
      else s = 0;
      t = (b * s + f) / e;
      if (t < 0) { t = 0; s = -c / a; s = s < 0 ? 0 : (s > 1 ? 1 : s); }
      else if (t > 1) { t = 1; s = (b - c) / a; s = s < 0 ? 0 : (s > 1 ? 1 : s); }
    }
  }
  for (int k = 0; k < 3; ++k) { c1[k] = p1[k] + d1[k] * s; c2[k] = p2[k] + d2[k] * t; }
}

/* ---- height field (bullet_objects.py:338-441: createCollisionShape(GEOM_HEIGHTFIELD, meshScale [1/scale, 1/scale, 1]), body placed at
 * z = (max + min) / 2 so that world heights are the data values).  btHeightfieldTerrainShape centres the grid on the origin: grid point
 * (ix, iy) sits at x = (ix - (cols - 1) / 2) / scale, y = (iy - (rows - 1) / 2) / scale, height data[iy * cols + ix]; every cell is two
 * triangles split along the diagonal from (ix + 1, iy) to (ix, iy + 1) (no flipQuadEdges, no diamond subdivision)  [UNVERIFIED-BULLET].
 * Outside the grid there is no terrain ("free falling off terrain", env_locomotion.py:1108). */
static void closest_on_triangle(const real *p, const real *a, const real *b, const real *c, real *q) { /* Ericson, Real-Time Collision Detection 5.1.5 */
  real ab[3], ac[3], ap[3], bp[3], cp[3];
  for (int k = 0; k < 3; ++k) { ab[k] = b[k] - a[k]; ac[k] = c[k] - a[k]; ap[k] = p[k] - a[k]; }
  real d1 = dot3(ab, ap), d2 = dot3(ac, ap);
  if (d1 <= 0 && d2 <= 0) { for (int k = 0; k < 3; ++k) q[k] = a[k]; return; }
  for (int k = 0; k < 3; ++k) bp[k] = p[k] - b[k];
  real d3 = dot3(ab, bp), d4 = dot3(ac, bp);
  if (d3 >= 0 && d4 <= d3) { for (int k = 0; k < 3; ++k) q[k] = b[k]; return; }
  real vc = d1 * d4 - d3 * d2;
  if (vc <= 0 && d1 >= 0 && d3 <= 0) { real v = d1 / (d1 - d3); for (int k = 0; k < 3; ++k) q[k] = a[k] + v * ab[k]; return; }
  for (int k = 0; k < 3; ++k) cp[k] = p[k] - c[k];
  real d5 = dot3(ab, cp), d6 = dot3(ac, cp);
  if (d6 >= 0 && d5 <= d6) { for (int k = 0; k < 3; ++k) q[k] = c[k]; return; }
  real vb = d5 * d2 - d1 * d6;
  if (vb <= 0 && d2 >= 0 && d6 <= 0) { real w = d2 / (d2 - d6); for (int k = 0; k < 3; ++k) q[k] = a[k] + w * ac[k]; return; }
  real va = d3 * d6 - d5 * d4;
  if (va <= 0 && (d4 - d3) >= 0 && (d5 - d6) >= 0) {
    real w = (d4 - d3) / ((d4 - d3) + (d5 - d6));
    for (int k = 0; k < 3; ++k) q[k] = b[k] + w * (c[k] - b[k]);
    return;
  }
  real den = 1 / (va + vb + vc), v = vb * den, w = vc * den;
  for (int k = 0; k < 3; ++k) q[k] = a[k] + ab[k] * v + ac[k] * w;
}
/* signed gap and world normal of a sphere against the height field.  Centre ABOVE the surface (z >= the piecewise-linear height under it,
 * or no surface under it): distance to the closest of the (up to) eight triangles of the 2 x 2 cells around the grid point nearest to the
 * centre (exact while radius + margin <= half a cell), normal from the closest point to the centre.  Centre BELOW the surface (a sphere
 * pushed more than its radius into the ground): signed distance to the plane of the triangle it is under, that triangle's normal.
 * Returns 1e30 where there is no terrain. */
/* the search window of a sphere of reach radius + margin: every cell it can touch lies within W = ceil(reach x scale + 1/2) cells of the grid
 * point nearest to its centre (the centre is at most half a cell from that point; 1e-6: a reach of exactly half a cell is W = 1).  Evaluated in
 * double precision by both sides (mocca_set_heightfield computes the kernel's per slot). */
static int hf_window(const Oracle *o, double reach) {
  int w = (int)ceil(reach * o->hf_scale + 0.5 - 1e-6);
  return w < 1 ? 1 : (w > 4 ? 4 : w);
}
static real sphere_heightfield(const Oracle *o, const real *C, real rad, int W, real *n) {
  const int cols = o->hf_cols, rows = o->hf_rows;
  const real sc = (real)o->hf_scale, cell = 1 / sc;
  real gap = 1e30;
  n[0] = 0; n[1] = 0; n[2] = 1;
  if (!o->hf) return gap;
  real fx = C[0] * sc + (real)0.5 * (cols - 1), fy = C[1] * sc + (real)0.5 * (rows - 1);
  if (!(fx >= -1 && fx <= cols && fy >= -1 && fy <= rows)) return gap;
  int iv = (int)floor(fx + (real)0.5), jv = (int)floor(fy + (real)0.5);
  int ic = (int)floor(fx), jc = (int)floor(fy); /* the cell the centre is over */
  /* centre below the surface: the plane of the triangle it is under (that cell is one of the central 2 x 2) */
  if (ic >= 0 && jc >= 0 && ic <= cols - 2 && jc <= rows - 2) {
    int i = ic, j = jc;
    real x0 = (i - (real)0.5 * (cols - 1)) * cell, y0 = (j - (real)0.5 * (rows - 1)) * cell;
    real v00[3] = {x0, y0, o->hf[j * cols + i]}, v10[3] = {x0 + cell, y0, o->hf[j * cols + i + 1]};
    real v01[3] = {x0, y0 + cell, o->hf[(j + 1) * cols + i]}, v11[3] = {x0 + cell, y0 + cell, o->hf[(j + 1) * cols + i + 1]};
    real u = fx - i, v = fy - j;
    const real *a = (u + v <= 1) ? v00 : v10, *b = (u + v <= 1) ? v10 : v11, *c = v01;
    real e1[3], e2[3], tn[3];
    for (int k = 0; k < 3; ++k) { e1[k] = b[k] - a[k]; e2[k] = c[k] - a[k]; }
    cross3(e1, e2, tn); /* counter-clockwise seen from above: points up */
    real il = 1 / sqrt(dot3(tn, tn));
    for (int k = 0; k < 3; ++k) tn[k] *= il;
    real side = (C[0] - a[0]) * tn[0] + (C[1] - a[1]) * tn[1] + (C[2] - a[2]) * tn[2];
    if (side < 0) { n[0] = tn[0]; n[1] = tn[1]; n[2] = tn[2]; return side - rad; }
  }
  for (int dj = -W; dj < W; ++dj)
    for (int di = -W; di < W; ++di) {
      int i = iv + di, j = jv + dj;
      if (i < 0 || j < 0 || i > cols - 2 || j > rows - 2) continue;
      real x0 = (i - (real)0.5 * (cols - 1)) * cell, y0 = (j - (real)0.5 * (rows - 1)) * cell;
      real v00[3] = {x0, y0, o->hf[j * cols + i]}, v10[3] = {x0 + cell, y0, o->hf[j * cols + i + 1]};
      real v01[3] = {x0, y0 + cell, o->hf[(j + 1) * cols + i]}, v11[3] = {x0 + cell, y0 + cell, o->hf[(j + 1) * cols + i + 1]};
      for (int t = 0; t < 2; ++t) {
        const real *a = t == 0 ? v00 : v10, *b = t == 0 ? v10 : v11, *c = v01;
        real q[3], d[3];
        closest_on_triangle(C, a, b, c, q);
        for (int k = 0; k < 3; ++k) d[k] = C[k] - q[k];
        real d2 = dot3(d, d), dist = sqrt(d2);
        if (dist - rad < gap) {
          gap = dist - rad;
          if (d2 > (real)1e-18) { n[0] = d[0] / dist; n[1] = d[1] / dist; n[2] = d[2] / dist; }
          else {
            real e1[3], e2[3], tn[3];
            for (int k = 0; k < 3; ++k) { e1[k] = b[k] - a[k]; e2[k] = c[k] - a[k]; }
            cross3(e1, e2, tn);
            real il = 1 / sqrt(dot3(tn, tn));
            n[0] = tn[0] * il; n[1] = tn[1] * il; n[2] = tn[2] * il;
          }
        }
      }
    }
  return gap;
}
/* HeightField.get_height_at (bullet_objects.py:348-353): ox, oy = data_size / scale / 2; data2d[int((y + oy) * scale), int((x + ox) * scale)]
 * (indices clamped to the grid here; the reference would wrap negative ones and raise past the end) */
static real hf_height_at(const Oracle *o, real x, real y) {
  if (!o->hf) return 0;
  real ox = (real)o->hf_rows / (real)o->hf_scale / 2, oy = (real)o->hf_cols / (real)o->hf_scale / 2;
  int ix = (int)((x + ox) * (real)o->hf_scale), iy = (int)((y + oy) * (real)o->hf_scale);
  ix = ix < 0 ? 0 : (ix > o->hf_cols - 1 ? o->hf_cols - 1 : ix);
  iy = iy < 0 ? 0 : (iy > o->hf_rows - 1 ? o->hf_rows - 1 : iy);
  return o->hf[iy * o->hf_cols + ix];
}

static void plank_frame(const Oracle *o, const Terrain *tr, int k, real *bc, real *Rb) {
  const MoccaModel *m = &o->m;
  const real *ti = tr->terrain[tr->plank_info[k]];
  /* set_step_state: quat = Euler(x_tilt, y_tilt, phi), env_locomotion.py:461-465 */
  euler_to_mat(ti[4], ti[5], ti[3], Rb);
  /* BaseStep.set_position (bullet_objects.py:77-83) puts the base link's inertial frame at
   * pos + _pos_offset with _pos_offset = (0,0,plank_com_z) NOT rotated by the plank orientation;
   * the slab centre sits half a thickness below the plank frame origin (the top face). */
  real cz = m->plank_com_z;
  real dn[3] = {0, 0, -(real)m->plank_half[2] - cz}, off[3];
  matvec3(Rb, dn, off);
  for (int i = 0; i < 3; ++i) bc[i] = ti[i] + off[i];
  bc[2] += cz;
}

static void collide(const Oracle *o, const Dyn *s, const Task *tk, const Terrain *tr, Work *w) {
  const MoccaModel *m = &o->m;
  w->nc = 0;
  for (int k = 0; k < m->n_feet; ++k) w->foot_touch[k] = w->foot_target[k] = 0;
  w->cover = 0;
  w->body_touch = 0;
  uint64_t slot_mask = 0;
  int n_self = 0;
  /* margins: Bullet's relative contact breaking threshold of the geom's link (MoccaModel.slot_margin / pair_margin, include/mocca_model.h) */
  /* terrain: every slot within the margin is a candidate; when there are more than the solver holds (a robot lying on the
   * ground) the max_contacts DEEPEST are kept (ties: lower slot first) and solved in slot order */
  typedef struct { int body, slot; real n[3], P[3], depth, mu, erp, cfm; } TerrainCand;
  TerrainCand cand[MOCCA_MAX_SLOTS];
  int ncand = 0;
  for (int g = 0; g < m->n_geoms; ++g) {
    if (!m->g_terrain[g]) continue;
    int ne = m->g_type[g] == MOCCA_GEOM_CAPSULE ? 2 : 1;
    for (int e = 0; e < ne; ++e) {
      real C[3], Cw[3], n[3] = {0, 0, 1}, gap, rad = m->g_radius[g];
      real mu, erp = m->erp, cfm = 0;
      int is_target = 0, cover_k = -1;
      geom_point(m, w, g, e, C);
      for (int k = 0; k < 3; ++k) Cw[k] = C[k] + s->pos[k];
      if (o->task_id == MOCCA_TASK_WALKER3D_PLANNER) {
        gap = sphere_heightfield(o, Cw, rad, hf_window(o, (double)(float)rad + (double)m->slot_margin[m->g_slot[g] + e]), n);
        mu = (real)m->plank_friction * (real)m->g_friction[g]; /* HeightField.reload: lateralFriction 1.0, contactStiffness 30000, contactDamping 1000 */
        real kk = m->plank_stiffness, cc = m->plank_damping, dt = m->dt;
        erp = dt * kk / (dt * kk + cc);
        cfm = 1 / (dt * kk + cc) / dt;
      } else if (o->task_id != MOCCA_TASK_WALKER3D_STEPPER) {
        gap = Cw[2] - rad;
        if (w->precise & 2) {
          int b = m->g_body[g];
          const float *pl = e ? m->g_p2[g] : m->g_p1[g];
          double zd = w->rd[b][2] + w->Rd[b][6] * pl[0] + w->Rd[b][7] * pl[1] + w->Rd[b][8] * pl[2] + (double)s->pos[2];
          gap = (real)(zd - (double)rad);
        }
        mu = (real)m->ground_friction * (real)m->g_friction[g];
      } else {
        gap = 1e30;
        real h[3] = {m->plank_half[0], m->plank_half[1], m->plank_half[2]};
        for (int k = 0; k < m->n_planks; ++k) {
          real bc[3], Rb[9], nn[3];
          plank_frame(o, tr, k, bc, Rb);
          real gk = m->plank_shape == MOCCA_PLANK_CYLINDER ? sphere_cylinder(Cw, rad, bc, Rb, h, nn) : sphere_box(Cw, rad, bc, Rb, h, nn);
          if (gk < gap) {
            gap = gk;
            n[0] = nn[0]; n[1] = nn[1]; n[2] = nn[2];
            /* cover link = top 1/10 of the slab (plank_large.urdf:40,49): contact with the target
             * plank's cover is what calc_feet_state tests (env_locomotion.py:634-650) */
            real d[3] = {Cw[0] - rad * nn[0] - bc[0], Cw[1] - rad * nn[1] - bc[1], Cw[2] - rad * nn[2] - bc[2]};
            real lz = Rb[2] * d[0] + Rb[5] * d[1] + Rb[8] * d[2];
            int cover = lz >= (real)m->plank_half[2] * (real)0.8;
            is_target = cover && (k == tk->next_step_index % m->n_planks);
            cover_k = cover ? k : -1;
          }
        }
        mu = (real)m->plank_friction * (real)m->g_friction[g];
        real kk = m->plank_stiffness, cc = m->plank_damping, dt = m->dt;
        erp = dt * kk / (dt * kk + cc);
        cfm = 1 / (dt * kk + cc) / dt;
      }
      if (gap < (real)m->slot_margin[m->g_slot[g] + e]) {
        slot_mask |= (uint64_t)1 << (m->g_slot[g] + e);
        if (o->task_id == MOCCA_TASK_WALKER3D_PLANNER) { if (m->g_torso[g]) w->body_touch = 1; } /* the torso link touches the terrain, :1104-1110 */
        else if (m->g_foot[g] >= 0) {
          w->foot_touch[m->g_foot[g]] = 1;
          if (is_target) w->foot_target[m->g_foot[g]] = 1;
          if (cover_k >= 0) w->cover |= 1 << (4 * m->g_foot[g] + cover_k);
        }
        else w->body_touch = 1; /* a non-foot link on the terrain (LaikagoCustomEnv, env_locomotion.py:880-890) */
        if (ncand < MOCCA_MAX_SLOTS) {
          TerrainCand *q = &cand[ncand++];
          q->body = m->g_body[g]; q->slot = m->g_slot[g] + e;
          for (int k = 0; k < 3; ++k) { q->n[k] = n[k]; q->P[k] = C[k] - rad * n[k]; }
          q->depth = -gap; q->mu = mu; q->erp = erp; q->cfm = cfm;
        }
      }
    }
  }
  /* contact manifolds (MoccaModel.manifold_max): per link at most four of its terrain candidates survive -- the deepest (ties: lower slot),
   * the one farthest from it, and the farthest on either side of the line through those two (signed area about the deepest point's normal) */
  if (m->manifold_max > 0) {
    int drop[MOCCA_MAX_SLOTS] = {0}, seen[MB] = {0};
    for (int i0 = 0; i0 < ncand; ++i0) {
      int b0 = cand[i0].body, cnt = 0;
      if (seen[b0]) continue;
      seen[b0] = 1;
      for (int i = 0; i < ncand; ++i) cnt += cand[i].body == b0;
      if (cnt <= 4) continue;
      int l1 = -1, l2 = -1, l3 = -1, l4 = -1;
      for (int i = 0; i < ncand; ++i) if (cand[i].body == b0 && (l1 < 0 || cand[i].depth > cand[l1].depth)) l1 = i;
      real dd2 = -1e30;
      for (int i = 0; i < ncand; ++i) {
        if (cand[i].body != b0 || i == l1) continue;
        real d[3] = {cand[i].P[0] - cand[l1].P[0], cand[i].P[1] - cand[l1].P[1], cand[i].P[2] - cand[l1].P[2]};
        real dd = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
        if (dd > dd2) { dd2 = dd; l2 = i; }
      }
      real e[3] = {cand[l2].P[0] - cand[l1].P[0], cand[l2].P[1] - cand[l1].P[1], cand[l2].P[2] - cand[l1].P[2]};
      real mp = 0, mm = 0;
      for (int i = 0; i < ncand; ++i) {
        if (cand[i].body != b0 || i == l1 || i == l2) continue;
        real d[3] = {cand[i].P[0] - cand[l1].P[0], cand[i].P[1] - cand[l1].P[1], cand[i].P[2] - cand[l1].P[2]}, cx[3];
        cross3(d, e, cx);
        real sg = cand[l1].n[0] * cx[0] + cand[l1].n[1] * cx[1] + cand[l1].n[2] * cx[2];
        if (sg > mp) { mp = sg; l3 = i; }
        if (-sg > mm) { mm = -sg; l4 = i; }
      }
      for (int i = 0; i < ncand; ++i)
        if (cand[i].body == b0 && i != l1 && i != l2 && i != l3 && i != l4) drop[i] = 1;
    }
    int k = 0;
    for (int i = 0; i < ncand; ++i)
      if (!drop[i]) cand[k++] = cand[i];
      else slot_mask &= ~((uint64_t)1 << cand[i].slot);
    ncand = k;
  }
  for (int i = 0; i < ncand; ++i) {
    int deeper = 0;
    for (int j = 0; j < ncand; ++j)
      if (cand[j].depth > cand[i].depth || (cand[j].depth == cand[i].depth && j < i)) ++deeper;
    if (ncand > m->max_contacts && deeper >= m->max_contacts) continue;
    int k = w->nc++;
    w->c_a[k] = cand[i].body; w->c_b[k] = -1; w->c_slot[k] = cand[i].slot;
    for (int x = 0; x < 3; ++x) { w->c_n[k][x] = cand[i].n[x]; w->c_P[k][x] = cand[i].P[x]; }
    w->c_depth[k] = cand[i].depth; w->c_mu[k] = cand[i].mu; w->c_erp[k] = cand[i].erp; w->c_cfm[k] = cand[i].cfm;
  }
  /* self collisions */
  for (int k = 0; k < m->n_pairs; ++k) {
    int ga = m->pair_a[k], gb = m->pair_b[k];
    real a1[3], a2[3], b1[3], b2[3], ca[3], cb[3];
    geom_point(m, w, ga, 0, a1); geom_point(m, w, ga, 1, a2);
    geom_point(m, w, gb, 0, b1); geom_point(m, w, gb, 1, b2);
    seg_seg(a1, a2, b1, b2, ca, cb);
    real d[3] = {ca[0] - cb[0], ca[1] - cb[1], ca[2] - cb[2]};
    real dist = sqrt(dot3(d, d)), ra = m->g_radius[ga], rb = m->g_radius[gb];
    real gap = dist - ra - rb, margin = m->pair_margin[k];
    if (gap < margin && w->nc < m->max_contacts && dist > (real)1e-9) {
      int i = w->nc++;
      w->c_a[i] = m->g_body[ga]; w->c_b[i] = m->g_body[gb]; w->c_slot[i] = -1;
      for (int j = 0; j < 3; ++j) {
        w->c_n[i][j] = d[j] / dist;
        /* midpoint between the two surface points */
        w->c_P[i][j] = (real)0.5 * ((ca[j] - ra * d[j] / dist) + (cb[j] + rb * d[j] / dist));
      }
      w->c_depth[i] = -gap; w->c_mu[i] = (real)m->g_friction[ga] * (real)m->g_friction[gb];
      w->c_erp[i] = m->erp; w->c_cfm[i] = 0;
    }
    if (gap < margin && dist > (real)1e-9) ++n_self;
    if (gap < margin && dist > (real)1e-9 && o->task_id == MOCCA_TASK_WALKER3D_PLANNER && (m->g_torso[ga] || m->g_torso[gb]))
      w->body_touch = 1; /* getContactPoints(linkIndexA=torso) reports contacts with the robot's own links too */
    /* Walker3DStepperEnv.calc_feet_state counts ANY contact of a foot link (env_locomotion.py:645-647) */
    if (gap < margin && dist > (real)1e-9 && o->task_id == MOCCA_TASK_WALKER3D_STEPPER)
      for (int f = 0; f < m->n_feet; ++f)
        if (m->g_body[ga] == m->foot_body[f] || m->g_body[gb] == m->foot_body[f]) w->foot_touch[f] = 1;
  }
  w->dbg[3] = (int32_t)(uint32_t)slot_mask; w->dbg[4] = (int32_t)(uint32_t)(slot_mask >> 32); w->dbg[7] = n_self;
  w->nc_wanted = ncand + n_self;
}

/* ------------------------------------------------------------------ */
/* constraint rows + PGS                                               */
/* ------------------------------------------------------------------ */
/* row Jacobian of  dir . (velocity of point Pa of body ba  -  velocity of point Pb of body bb)  ; bb < 0: world */
static void pair_jacobian(const MoccaModel *m, const Work *w, int ba, const real *Pa, int bb, const real *Pb, const real *dir,
                          real *J) {
  int nd = 6 + m->n_joints;
  real F[6], pn[3];
  cross3(Pa, dir, pn);
  for (int k = 0; k < 3; ++k) { F[k] = pn[k]; F[3 + k] = dir[k]; }
  for (int k = 0; k < nd; ++k) J[k] = 0;
  for (int k = 0; k < 6; ++k) J[k] = F[k];
  for (int b = 1; b < m->n_bodies; ++b)
    if (m->anc_mask[ba] & (1u << b)) J[5 + b] = dot6(w->S[b], F);
  if (bb >= 0) {
    cross3(Pb, dir, pn);
    for (int k = 0; k < 3; ++k) { F[k] = pn[k]; F[3 + k] = dir[k]; }
    for (int k = 0; k < 6; ++k) J[k] -= F[k];
    for (int b = 1; b < m->n_bodies; ++b)
      if (m->anc_mask[bb] & (1u << b)) J[5 + b] -= dot6(w->S[b], F);
  }
}
static void contact_jacobian(const MoccaModel *m, const Work *w, int ba, int bb, const real *P, const real *dir, real *J) {
  pair_jacobian(m, w, ba, P, bb, P, dir, J);
}

/* nu = [omega(3) v(3) qd(by body, at 5+b)] */
static void solve_constraints(const MoccaModel *m, Dyn *s, Work *w, real *nu) {
  int nd = 6 + m->n_joints, nr = 0;
  real dt = m->dt, idt = 1 / dt;
  /* --- joint limit rows first (Bullet solves non-contact rows first) --- */
  uint64_t limit_mask = 0;
  for (int b = 1; b < m->n_bodies; ++b) {
    for (int side = 0; side < 2; ++side) {
      real sgn = side == 0 ? 1 : -1;
      real gap = side == 0 ? s->q[b] - (real)m->jlo[b] : (real)m->jhi[b] - s->q[b];
      real vel = sgn * nu[5 + b];
      if (m->limit_at_violation ? gap > 0 : gap + dt * vel >= (real)m->limit_slack) continue;
      limit_mask |= (uint64_t)1 << (2 * (b - 1) + side);
      if (nr >= m->max_rows) continue;
      int r = nr++;
      for (int k = 0; k < nd; ++k) w->J[r][k] = 0;
      w->J[r][5 + b] = sgn;
      w->row_kind[r] = 0; w->row_normal[r] = -1; w->row_mu[r] = 0; w->row_slot[r] = -1;
      w->bias[r] = gap < 0 ? (real)m->erp_noncontact * (-gap) * idt : -gap * idt;
      w->cfm[r] = 0; w->lam[r] = 0;
    }
  }
  /* --- point-to-point loop closures (bilateral, 3 rows each), env_cassie.py:114-137 --- */
  for (int c = 0; c < m->n_closures; ++c) {
    int ba = m->cl_body_a[c], bb = m->cl_body_b[c];
    real la[3] = {m->cl_point_a[c][0], m->cl_point_a[c][1], m->cl_point_a[c][2]};
    real lb[3] = {m->cl_point_b[c][0], m->cl_point_b[c][1], m->cl_point_b[c][2]}, Pa[3], Pb[3];
    matvec3(w->R[ba], la, Pa); matvec3(w->R[bb], lb, Pb);
    for (int k = 0; k < 3; ++k) { Pa[k] += w->r[ba][k]; Pb[k] += w->r[bb][k]; }
    for (int ax = 0; ax < 3 && nr < m->max_rows; ++ax) {
      real dir[3] = {ax == 0, ax == 1, ax == 2};
      int r = nr++;
      pair_jacobian(m, w, ba, Pa, bb, Pb, dir, w->J[r]);
      w->row_kind[r] = 3; w->row_normal[r] = -1; w->row_mu[r] = 0; w->row_slot[r] = -1;
      real gap_ = Pb[ax] - Pa[ax];
      if (w->precise & 1) {
        double pa = w->rd[ba][ax], pb = w->rd[bb][ax];
        for (int k = 0; k < 3; ++k) { pa += w->Rd[ba][3 * ax + k] * m->cl_point_a[c][k]; pb += w->Rd[bb][3 * ax + k] * m->cl_point_b[c][k]; }
        gap_ = (real)(pb - pa);
      }
      w->bias[r] = (real)m->erp_noncontact * gap_ * idt; /* pull pivot a onto pivot b */
      w->cfm[r] = 0; w->lam[r] = 0;
    }
  }
  /* --- CassieEnv(planar=True), env_cassie.py:326-341: the base is held in the x-z plane by three bilateral rows on
   *     nu = [omega; v]: omega_x, omega_z (the base's y axis stays the world's: small-angle error of R e_y) and v_y --- */
  int n_planar = 0;
  if (m->planar) {
    const real *R0 = w->R[0];
    real err[3] = {R0[7], -R0[1], s->pos[1] - (real)m->init_pos[1]};
    if (w->precise & 4) { err[0] = (real)w->Rd[0][7]; err[1] = (real)-w->Rd[0][1]; }
    int comp[3] = {0, 2, 4};
    for (int k = 0; k < 3 && nr < m->max_rows; ++k) {
      int r = nr++;
      for (int c = 0; c < nd; ++c) w->J[r][c] = 0;
      w->J[r][comp[k]] = 1;
      w->row_kind[r] = 3; w->row_normal[r] = -1; w->row_mu[r] = 0; w->row_slot[r] = -1;
      w->bias[r] = -(real)m->erp_noncontact * err[k] * idt;
      w->cfm[r] = 0; w->lam[r] = 0;
      ++n_planar;
    }
  }
  /* --- contact normals, then friction pairs --- */
  int first_normal = nr;
  int nc = w->nc;
  if (nc > (m->max_rows - nr) / 3) nc = (m->max_rows - nr) / 3;
  for (int i = 0; i < nc; ++i) {
    int r = nr++;
    contact_jacobian(m, w, w->c_a[i], w->c_b[i], w->c_P[i], w->c_n[i], w->J[r]);
    w->row_kind[r] = 1; w->row_normal[r] = -1; w->row_mu[r] = 0; w->row_slot[r] = w->c_slot[i];
    real depth = w->c_depth[i] - (real)m->linear_slop; /* penetration = distance + m_linearSlop [UNVERIFIED-BULLET]; 0 in the compiled blobs */
    w->bias[r] = depth > 0 ? w->c_erp[i] * depth * idt : depth * idt;
    w->cfm[r] = w->c_cfm[i];
    w->lam[r] = (w->c_slot[i] >= 0) ? (real)m->warmstart * s->warm[w->c_slot[i]] : 0;
  }
  for (int i = 0; i < nc; ++i) {
    real t1[3], t2[3];
    plane_space(w->c_n[i], t1, t2);
    for (int dsel = 0; dsel < 2; ++dsel) {
      int r = nr++;
      contact_jacobian(m, w, w->c_a[i], w->c_b[i], w->c_P[i], dsel ? t2 : t1, w->J[r]);
      w->row_kind[r] = 2; w->row_normal[r] = first_normal + i; w->row_mu[r] = w->c_mu[i]; w->row_slot[r] = -1;
      w->bias[r] = 0; w->cfm[r] = 0; w->lam[r] = 0;
    }
  }
  w->nr = nr;
  w->dbg[0] = nr; w->dbg[1] = first_normal - 3 * m->n_closures - n_planar; w->dbg[2] = nc;
  w->dbg[5] = (int32_t)(uint32_t)limit_mask; w->dbg[6] = (int32_t)(uint32_t)(limit_mask >> 32);
  { /* cap pressure of this substep (MOCCA_DBG_CAP_*): Bullet has neither cap */
    int nl_raw = __builtin_popcountll(limit_mask), nfix = 3 * m->n_closures + (m->planar ? 3 : 0);
    int kept = w->nc_wanted < m->max_contacts ? w->nc_wanted : m->max_contacts;
    w->dbg[12] = w->nc_wanted > m->max_contacts;
    w->dbg[13] = nl_raw + nfix + 3 * kept > m->max_rows;
    w->dbg[14] = 1;
    w->dbg[15] = nl_raw + nfix + 3 * w->nc_wanted;
  }
  /* --- responses, Delassus matrix, initial velocities --- */
  for (int r = 0; r < nr; ++r) minv_apply(m, w, w->J[r], w->Mi[r]);
  for (int r = 0; r < nr; ++r)
    for (int c = 0; c < nr; ++c) {
      real a = 0;
      for (int k = 0; k < nd; ++k) a += w->J[r][k] * w->Mi[c][k];
      w->A[r][c] = a;
    }
  for (int r = 0; r < nr; ++r) {
    real a = 0;
    for (int k = 0; k < nd; ++k) a += w->J[r][k] * nu[k];
    w->w[r] = a;
  }
  /* warm-start impulses act before the first iteration */
  for (int r = 0; r < nr; ++r)
    if (w->lam[r] != 0)
      for (int c = 0; c < nr; ++c) w->w[c] += w->A[r][c] * w->lam[r];
  /* --- projected Gauss-Seidel --- */
  uint64_t clamp_sig = 0, clamp_last = 0; /* MOCCA_DBG_CLAMP*: rows left ON a bound, by the HIP solver's lane numbers */
  int first_fric = first_normal + nc;
  for (int it = 0; it < m->n_iters; ++it) {
    clamp_last = 0;
    /* MoccaModel.sweep_alternate: the rows that are not contacts (limits, closures, planar rows: 0 .. first_normal - 1) are visited LAST TO FIRST
     * in the even iterations and first to last in the odd ones -- btMultiBodyConstraintSolver::solveSingleIteration: `index = iteration & 1 ? j
     * : size - 1 - j` over m_multiBodyNonContactConstraints; contact normals and friction rows always forward  [UNVERIFIED-BULLET] */
    const int rev = m->sweep_alternate && !(it & 1);
    for (int ro = 0; ro < nr; ++ro) {
      int r = (rev && ro < first_normal) ? first_normal - 1 - ro : ro;
      if (m->friction_cone && w->row_kind[r] == 2) {
        /* Implicit cone friction (btMultiBodyConstraintSolver::resolveConeFrictionConstraintRows): the contact's two friction rows r, r + 1
         * take their candidate impulses from the SAME velocity state, the pair is clipped to the circle of radius mu * lambda_n (Bullet:
         * angle = atan2(sumA, sumB), |sumA| <= lim |sin|, |sumB| <= lim |cos| -- the radial projection), then both deltas are applied. */
        int rb = r + 1;
        real lam_n = w->lam[w->row_normal[r]], lim = w->row_mu[r] * lam_n;
        if (lam_n > 0) { /* Bullet: `if (totalImpulse > btScalar(0))` -- without a normal impulse the friction rows are left as they are */
          real s2[2];
          for (int k = 0; k < 2; ++k) {
            int q = r + k;
            real den = w->A[q][q] + w->cfm[q];
            s2[k] = w->lam[q] + (den > (real)1e-12 ? (w->bias[q] - w->w[q] - w->cfm[q] * w->lam[q]) / den : 0);
          }
          real r2 = s2[0] * s2[0] + s2[1] * s2[1];
          real sc = r2 > lim * lim ? lim / (real)sqrt(r2) : 1;
          for (int k = 0; k < 2; ++k) {
            int q = r + k;
            real nl = s2[k] * sc, dl = nl - w->lam[q];
            w->lam[q] = nl;
            if (dl != 0)
              for (int c = 0; c < nr; ++c) w->w[c] += w->A[q][c] * dl;
          }
        }
        {
          /* "on the bound": the pair sits on the circle (1e-5 relative; the HIP solver evaluates the same expression after the sweep) */
          real l2 = w->lam[r] * w->lam[r] + w->lam[rb] * w->lam[rb];
          int clamped = l2 >= lim * lim * (real)(1 - 1e-5);
          for (int k = 0; k < 2; ++k) {
            int q = r + k, lane = KERNEL_MAXR(m) - 2 - 2 * ((q - first_fric) / 2) + ((q - first_fric) & 1);
            if (clamped) clamp_last |= (uint64_t)1 << lane;
          }
        }
        ++ro;
        continue;
      }
      real lo = 0, hi = (real)1e30;
      if (w->row_kind[r] == 3) lo = (real)-1e30;
      if (w->row_kind[r] == 2) {
        real lim = w->row_mu[r] * w->lam[w->row_normal[r]];
        lo = -lim; hi = lim;
      }
      /* a row whose Jacobian vanishes (e.g. the out-of-plane friction direction of a self contact of a planar
       * mechanism) has A_rr = 0: Bullet gives such a row a zero gain (jacDiagABInv = 0 when the denominator is below
       * SIMD_EPSILON) instead of dividing */
      real den = w->A[r][r] + w->cfm[r];
      real dl = den > (real)1e-12 ? (w->bias[r] - w->w[r] - w->cfm[r] * w->lam[r]) / den : 0;
      if (w->row_kind[r] == 2 && !(w->lam[w->row_normal[r]] > 0)) { dl = 0; lo = (real)-1e30; hi = (real)1e30; } /* pyramid: the same `if (totalImpulse > 0)` */
      real nl = w->lam[r] + dl;
      nl = nl < lo ? lo : (nl > hi ? hi : nl);
      dl = nl - w->lam[r];
      w->lam[r] = nl;
      if (dl != 0)
        for (int c = 0; c < nr; ++c) w->w[c] += w->A[r][c] * dl;
      {
        real hi_f = w->row_kind[r] == 2 ? w->row_mu[r] * w->lam[w->row_normal[r]] : 0;
        int clamped = w->row_kind[r] == 2 ? fabs(nl) == hi_f : (w->row_kind[r] != 3 && nl == 0);
        int lane = r < first_fric ? r : KERNEL_MAXR(m) - 2 - 2 * ((r - first_fric) / 2) + ((r - first_fric) & 1);
        if (clamped) clamp_last |= (uint64_t)1 << lane;
      }
    }
    clamp_sig = ((clamp_sig << 7) | (clamp_sig >> 57)) ^ clamp_last;
  }
  w->dbg[8] = (int32_t)(uint32_t)clamp_last; w->dbg[9] = (int32_t)(uint32_t)(clamp_last >> 32);
  w->dbg[10] = (int32_t)(uint32_t)clamp_sig; w->dbg[11] = (int32_t)(uint32_t)(clamp_sig >> 32);
  /* --- apply --- */
  for (int k = 0; k < nd; ++k) {
    real a = 0;
    for (int r = 0; r < nr; ++r) a += w->Mi[r][k] * w->lam[r];
    nu[k] += a;
  }
  for (int k = 0; k < m->n_slots; ++k) s->warm[k] = 0;
  for (int r = 0; r < nr; ++r)
    if (w->row_slot[r] >= 0) s->warm[w->row_slot[r]] = w->lam[r];
}

/* one physics substep: bullet_utils.py:352-353 stepSimulation() does n_substeps of these */
static void substep(const Oracle *o, Dyn *s, const Task *tk, const Terrain *tr, const real *tau, Work *w) {
  const MoccaModel *m = &o->m;
  real dt = m->dt;
  kinematics(m, s, w);
  if (w->precise) kinematics_d(m, s, w);
  collide(o, s, tk, tr, w);
  aba(m, s, tau, w, 1);
  real nu[NDOF_MAX];
  const real *a0 = w->acc[0];
  real wxv[3];
  cross3(s->omg, s->vel, wxv);
  for (int k = 0; k < 3; ++k) {
    nu[k] = s->omg[k] + dt * a0[k];
    nu[3 + k] = s->vel[k] + dt * (a0[3 + k] + wxv[k]); /* spatial -> classical acceleration */
  }
  for (int b = 1; b < m->n_bodies; ++b) nu[5 + b] = s->qd[b] + dt * w->qdd[b];
  solve_constraints(m, s, w, nu);
  for (int k = 0; k < 3; ++k) { s->omg[k] = nu[k]; s->vel[k] = nu[3 + k]; }
  for (int b = 1; b < m->n_bodies; ++b) {
    real v = nu[5 + b], mx = m->max_qd;
    v = v > mx ? mx : (v < -mx ? -mx : v);
    s->qd[b] = v;
    s->q[b] += dt * v;
  }
  for (int k = 0; k < 3; ++k) s->pos[k] += dt * s->vel[k];
  /* quaternion exponential map, world-frame omega */
  real wn = sqrt(dot3(s->omg, s->omg)), th = wn * dt, dq[4];
  if (th > (real)1e-8) {
    real sn = sin((real)0.5 * th) / wn;
    dq[0] = s->omg[0] * sn; dq[1] = s->omg[1] * sn; dq[2] = s->omg[2] * sn; dq[3] = cos((real)0.5 * th);
  } else {
    dq[0] = (real)0.5 * dt * s->omg[0]; dq[1] = (real)0.5 * dt * s->omg[1]; dq[2] = (real)0.5 * dt * s->omg[2]; dq[3] = 1;
  }
  real *q = s->quat, nq[4];
  nq[0] = dq[3] * q[0] + dq[0] * q[3] + dq[1] * q[2] - dq[2] * q[1];
  nq[1] = dq[3] * q[1] - dq[0] * q[2] + dq[1] * q[3] + dq[2] * q[0];
  nq[2] = dq[3] * q[2] + dq[0] * q[1] - dq[1] * q[0] + dq[2] * q[3];
  nq[3] = dq[3] * q[3] - dq[0] * q[0] - dq[1] * q[1] - dq[2] * q[2];
  real nn = 1 / sqrt(nq[0] * nq[0] + nq[1] * nq[1] + nq[2] * nq[2] + nq[3] * nq[3]);
  for (int k = 0; k < 4; ++k) q[k] = nq[k] * nn;
}

/* debug record of env `env` after a substep: words 0..11 = this substep's active set, 12..15 cumulative (include/mocca.h) */
static void dbg_commit(Oracle *o, int env, const Work *w) {
  int32_t *d = o->dbg + (size_t)DBG_WORDS * env;
  memcpy(d, w->dbg, 12 * sizeof(int32_t));
  d[12] += w->dbg[12]; d[13] += w->dbg[13]; d[14] += w->dbg[14];
  if (w->dbg[15] > d[15]) d[15] = w->dbg[15];
  /* step signature (MOCCA_DBG_STEPSIG_*): every substep's twelve words folded in order; restarted by dbg_step_start() */
  uint64_t h = ((uint64_t)(uint32_t)d[17] << 32) | (uint32_t)d[16];
  for (int k = 0; k < 12; ++k) h = (h ^ (uint64_t)(uint32_t)d[k]) * 0x9E3779B97F4A7C15ull;
  d[16] = (int32_t)(uint32_t)h; d[17] = (int32_t)(uint32_t)(h >> 32); d[18] += 1;
}
static void dbg_step_start(Oracle *o, int env) {
  int32_t *d = o->dbg + (size_t)DBG_WORDS * env;
  d[16] = 0; d[17] = 0; d[18] = 0;
}

/* ------------------------------------------------------------------ */
/* task layer                                                          */
/* ------------------------------------------------------------------ */
/* pybullet.getEulerFromQuaternion [UNVERIFIED-BULLET singularity handling], bullet_utils.py:84 */
static void quat_to_rpy(const real *q, real *rpy) {
  real x = q[0], y = q[1], z = q[2], w = q[3];
  real sarg = -2 * (x * z - w * y);
  if (sarg <= (real)-0.99999) { rpy[1] = (real)-1.5707963267948966; rpy[0] = 0; rpy[2] = 2 * atan2(x, -y); }
  else if (sarg >= (real)0.99999) { rpy[1] = (real)1.5707963267948966; rpy[0] = 0; rpy[2] = 2 * atan2(-x, y); }
  else {
    rpy[0] = atan2(2 * (y * z + w * x), w * w - x * x - y * y + z * z);
    rpy[1] = asin(sarg);
    rpy[2] = atan2(2 * (x * y + w * z), w * w + x * x - y * y - z * z);
  }
}

/* WalkerBase.calc_state, robots.py:42-95.  Needs kinematics() done on the current state.
 * Writes 6 + 2 nj + n_feet floats; returns joints_at_limit via *jal; speeds in `spd`. */
static void calc_robot_state(Oracle *o, const Dyn *s, const Task *tk, float *out, int *jal, float *spd) {
  const MoccaModel *m = &o->m;
  Work *w = &o->wk;
  int nj = m->n_joints, cnt = 0;
  for (int b = 1; b <= nj; ++b) {
    float ang = (float)s->q[b], lo = m->jlo[b], wt = m->jhi[b] - m->jlo[b]; /* robots.py:46,125-132 */
    float nrm = 2 * (ang - lo) / wt - 1;
    float sp = 0.1f * (float)s->qd[b];
    out[6 + b - 1] = nrm;
    out[6 + nj + b - 1] = sp;
    spd[b - 1] = sp;
    if (fabsf(nrm) > 0.99f) ++cnt;
  }
  *jal = cnt;
  quat_to_rpy(s->quat, o->body_rpy);
  real yaw = o->body_rpy[2], cy = cos(-yaw), sy = sin(-yaw);
  o->body_vel[0] = cy * s->vel[0] - sy * s->vel[1]; /* robots.py:63-70 */
  o->body_vel[1] = sy * s->vel[0] + cy * s->vel[1];
  o->body_vel[2] = s->vel[2];
  real minz = 1e30;
  for (int k = 0; k < m->n_feet; ++k) {
    int b = m->foot_body[k];
    real fp[3] = {m->foot_point[k][0], m->foot_point[k][1], m->foot_point[k][2]}, fw[3];
    matvec3(w->R[b], fp, fw); /* the foot LINK's centre of mass: getLinkState[0], bullet_utils.py:106 */
    for (int i = 0; i < 3; ++i) o->feet_xyz[k][i] = s->pos[i] + w->r[b][i] + fw[i];
    if (o->feet_xyz[k][2] < minz) minz = o->feet_xyz[k][2];
  }
  out[0] = (float)(s->pos[2] - minz); /* robots.py:88-89 */
  out[1] = (float)o->body_vel[0]; out[2] = (float)o->body_vel[1]; out[3] = (float)o->body_vel[2];
  out[4] = (float)o->body_rpy[0]; out[5] = (float)o->body_rpy[1];
  for (int k = 0; k < m->n_feet; ++k) out[6 + 2 * nj + k] = (float)tk->feet_contact[k];
  int n = 6 + 2 * nj + m->n_feet;
  for (int i = 0; i < n; ++i) out[i] = out[i] > 5.f ? 5.f : (out[i] < -5.f ? -5.f : out[i]); /* robots.py:95 */
}

/* calc_potential, env_locomotion.py:143-158 / :584-596 */
static void calc_potential(const Oracle *o, const Dyn *s, Task *tk, real *dist_out, real *ang_out) {
  real dx = tk->walk_target[0] - s->pos[0], dy = tk->walk_target[1] - s->pos[1];
  real theta = atan2(dy, dx);
  real ang = theta - o->body_rpy[2];
  real dist = sqrt(dx * dx + dy * dy);
  tk->linear_potential = -dist / (real)o->m.control_dt;
  tk->angular_potential = cos(ang);
  *dist_out = dist; *ang_out = ang;
}

static void randomize_target(Oracle *o, int env, Task *tk) { /* env_locomotion.py:67-74 */
  if (o->eval_mode) { tk->dist = 4; tk->angle = 0; }
  else {
    real u0 = draw_uniform(o, env, tk), u1 = draw_uniform(o, env, tk);
    tk->dist = 3 + 2 * u0;
    tk->angle = (real)-1.5707963267948966 + (real)3.141592653589793 * u1;
  }
  real u2 = draw_uniform(o, env, tk);
  tk->stop_frames = u2 < (real)0.5 ? 30 : 60;
}

static void softsign_tail(real dist, real ang, float *o2) { /* env_locomotion.py:102-105,124-127 */
  real s = dist * sin(ang), c = dist * cos(ang);
  o2[0] = (float)(s / (1 + fabs(s)));
  o2[1] = (float)(c / (1 + fabs(c)));
}

/* The blob stores the Stepper's class attributes (0.65, 0.45, 1.2 ...) as fp32; the reference computes with the decimal
 * itself.  DEC() recovers the 6-decimal number an fp32 constant renders, so the f64 build reproduces the reference to
 * 1e-9 instead of 1e-7 x (a step bonus of 50 amplifies that to 1e-5); in the f32 build it is the identity. */
#define DEC(x) ((real)(round((double)(x) * 1e6) / 1e6))

/* ---- stepper terrain, env_locomotion.py:395-441 (device RNG version) ---- */
static void generate_step_placements(Oracle *o, int env, Task *tk, Terrain *tr) {
  const MoccaModel *m = &o->m;
  const real DEG2RAD = (real)(3.14159265358979323846 / 180.0);
  int N = MOCCA_MAX_TERRAIN_STEPS, cur = tk->curriculum > 9 ? 9 : tk->curriculum;
  real ratio = (real)cur / 9;
  real d0 = DEC(m->dist_range[0]), d1 = DEC(m->dist_range[1]);
  real dist_lo = d0, dist_hi = d0 + (d1 - d0) * cur / 9; /* np.linspace(*dist_range, 10)[cur] */
  real yaw_lo = -(real)m->yaw_range_deg * ratio * DEG2RAD, yaw_hi = (real)m->yaw_range_deg * ratio * DEG2RAD;
  real pit_lo = -(real)m->pitch_range_deg * ratio * DEG2RAD + (real)1.5707963267948966, pit_hi = (real)m->pitch_range_deg * ratio * DEG2RAD + (real)1.5707963267948966;
  real tl_lo = -(real)m->tilt_range_deg * ratio * DEG2RAD, tl_hi = (real)m->tilt_range_deg * ratio * DEG2RAD;
  real dr[MOCCA_MAX_TERRAIN_STEPS], dphi[MOCCA_MAX_TERRAIN_STEPS], dth[MOCCA_MAX_TERRAIN_STEPS];
  real xt[MOCCA_MAX_TERRAIN_STEPS], yt[MOCCA_MAX_TERRAIN_STEPS];
  /* draw order = the five np_random.uniform(size=N) calls of env_locomotion.py:408-412 */
  for (int i = 0; i < N; ++i) dr[i] = dist_lo + (dist_hi - dist_lo) * draw_uniform(o, env, tk);
  for (int i = 0; i < N; ++i) dphi[i] = yaw_lo + (yaw_hi - yaw_lo) * draw_uniform(o, env, tk);
  for (int i = 0; i < N; ++i) dth[i] = pit_lo + (pit_hi - pit_lo) * draw_uniform(o, env, tk);
  for (int i = 0; i < N; ++i) xt[i] = tl_lo + (tl_hi - tl_lo) * draw_uniform(o, env, tk);
  for (int i = 0; i < N; ++i) yt[i] = tl_lo + (tl_hi - tl_lo) * draw_uniform(o, env, tk);
  dr[0] = 0; dphi[0] = 0; dth[0] = (real)1.5707963267948966;
  dr[1] = dr[2] = DEC(m->init_step_separation); dphi[1] = dphi[2] = 0; dth[1] = dth[2] = (real)1.5707963267948966;
  xt[0] = xt[1] = xt[2] = 0; yt[0] = yt[1] = yt[2] = 0;
  real x = 0, y = 0, z = 0, phi = 0;
  real dx_min = DEC(m->step_radius) * (real)2.5; /* :434-435 */
  for (int i = 0; i < N; ++i) {
    phi += dphi[i];
    real dx = dr[i] * sin(dth[i]) * cos(phi), dy = dr[i] * sin(dth[i]) * sin(phi), dz = dr[i] * cos(dth[i]);
    if (i >= 2) {
      real ax = fabs(dx), mx = ax > dx_min ? ax : dx_min;
      real sg = dx > 0 ? 1 : (dx < 0 ? -1 : 0);
      dx = sg * (mx < d1 ? mx : d1);
    }
    x += dx; y += dy; z += dz;
    tr->terrain[i][0] = x; tr->terrain[i][1] = y; tr->terrain[i][2] = z;
    tr->terrain[i][3] = phi; tr->terrain[i][4] = xt[i]; tr->terrain[i][5] = yt[i];
  }
}

/* delta_to_k_targets, env_locomotion.py:712-759 : 3 rows x (x,y,z,x_tilt,y_tilt), sets walk_target */
static void delta_to_k_targets(const Oracle *o, const Dyn *s, Task *tk, const Terrain *tr, float *out) {
  /* lookbehind j rows before the next step, then lookahead k = 2 rows from it; indices clamp at both ends ("repeat first /
   * last target", :717-734); stopping repeats the next step */
  int N = tk->next_step_index, T = MOCCA_MAX_TERRAIN_STEPS, j = o->m.lookbehind, nt = j + 2, idx[4];
  for (int i = 0; i < nt; ++i) {
    int v = N - j + i;
    if (tk->stop_on_next_step && i >= j) v = N;
    idx[i] = v < 0 ? 0 : (v > T - 1 ? T - 1 : v);
  }
  for (int i = 0; i < 3; ++i) tk->walk_target[i] = tr->terrain[idx[nt - 1]][i]; /* walk_target_index = -1 */
  for (int i = 0; i < nt; ++i) {
    const real *t = tr->terrain[idx[i]];
    real dx = t[0] - s->pos[0], dy = t[1] - s->pos[1], dz = t[2] - s->pos[2];
    real ang = atan2(dy, dx) - o->body_rpy[2], dist = sqrt(dx * dx + dy * dy);
    out[5 * i + 0] = (float)(sin(ang) * dist);
    out[5 * i + 1] = (float)(cos(ang) * dist);
    out[5 * i + 2] = (float)dz;
    out[5 * i + 3] = (float)t[4];
    out[5 * i + 4] = (float)t[5];
  }
}

static int obs_dim(const Oracle *o) {
  if (o->task_id == MOCCA_TASK_CASSIE) /* env_cassie.py:76-79,344-346; the phase envs: 40 + 2 (:574,633) */
    return o->m.cassie_mode == MOCCA_CASSIE_PLAIN ? 6 + 2 * o->m.n_ordered + 2 : 12 + 2 * o->m.n_ordered + 2;
  int base = 6 + 2 * o->m.n_joints + o->m.n_feet;
  return (o->task_id == MOCCA_TASK_WALKER3D_CUSTOM || o->task_id == MOCCA_TASK_WALKER3D_PLANNER) ? base + 2 : base + 5 * (o->m.lookbehind + 2);
}

/* ---------------- Cassie task layer, env_cassie.py:238-276,348-479; mocap / phase variants :481-660 ---------------- */
/* frame of the reference motion at mocap_time() = istep * control_step / llc_frame_skip (:359-360): the re-created
 * CassieTrajectory (mocca_envs_amd/trajectory.py) maps t to frame int((t mod T) / T * n) */
static int traj_frame(const Oracle *o, int istep, real *phase) {
  double t = (double)istep * o->traj_cstep / (double)o->m.n_llc, T = o->traj_tmax;
  if (phase) *phase = (real)fmod(t / T, 1.0); /* CassiePhaseMoccaEnv.get_obs, :639 */
  int i = (int)(fmod(t, T) / T * (double)o->traj_n);
  return i < o->traj_n - 1 ? i : o->traj_n - 1;
}
/* joint_angles[k]: Joint.current_relative_position (bullet_utils.py:212-216) cast to float32 (env_cassie.py:239-242) */
static float cassie_nrm(const MoccaModel *m, int k, real q) {
  int b = m->ordered_body[k];
  real lo = m->jlo[b], hi = m->jhi[b], mid = (real)0.5 * (lo + hi);
  return (float)(2 * (q - mid) / (hi - lo));
}
/* rad_joint_angles = to_radians(joint_angles) (:243,208-210) */
static real cassie_rad(const MoccaModel *m, int k, float nrm) {
  int b = m->ordered_body[k];
  real lo = m->jlo[b], hi = m->jhi[b];
  return (hi - lo) * ((real)nrm + 1) / 2 + lo;
}
/* Cassie.calc_state (:238-276); needs kinematics() done.  robot_state[34] as float32 like the reference; returns pelvis z - lowest toe z. */
static real cassie_state(Oracle *o, const Dyn *s, const Task *tk, float *rs) {
  const MoccaModel *m = &o->m;
  Work *w = &o->wk;
  int no = m->n_ordered;
  quat_to_rpy(s->quat, o->body_rpy);
  real yaw = o->body_rpy[2], cy = cos(-yaw), sy = sin(-yaw);
  o->body_vel[0] = cy * s->vel[0] - sy * s->vel[1];
  o->body_vel[1] = sy * s->vel[0] + cy * s->vel[1];
  o->body_vel[2] = s->vel[2];
  rs[0] = (float)(s->pos[2] - tk->initial_z);
  rs[1] = (float)o->body_vel[0];
  rs[2] = (float)o->body_vel[1];
  rs[3] = (float)o->body_vel[2];
  rs[4] = (float)o->body_rpy[0];
  rs[5] = (float)o->body_rpy[1];
  for (int k = 0; k < no; ++k) {
    rs[6 + k] = cassie_nrm(m, k, s->q[m->ordered_body[k]]);
    rs[6 + no + k] = (float)s->qd[m->ordered_body[k]];
  }
  /* the feet as the walkers read them (robot_state above): the blob's foot point on the foot link -- the link's centre of mass in the
   * compiled blob (model.compile_cassie), a field of its own in any blob, and the one the kernel reads */
  real minz = 1e30;
  for (int k = 0; k < m->n_feet; ++k) {
    int b = m->foot_body[k];
    real fp[3] = {m->foot_point[k][0], m->foot_point[k][1], m->foot_point[k][2]}, fw[3];
    matvec3(w->R[b], fp, fw);
    real z = s->pos[2] + w->r[b][2] + fw[2];
    if (z < minz) minz = z;
  }
  return s->pos[2] - minz;
}
/* CassieEnv.get_obs (:416-431) */
static void cassie_obs(Oracle *o, const Dyn *s, const float *rs, float *obs) {
  const MoccaModel *m = &o->m;
  int no = m->n_ordered;
  for (int i = 0; i < 6 + 2 * no; ++i) obs[i] = rs[i];
  real yaw = o->body_rpy[2];
  real dx = (real)m->cassie_target[0] - s->pos[0], dy = (real)m->cassie_target[1] - s->pos[1];
  real dth = atan2(dy, dx) - yaw, c = cos(dth), sn = sin(dth);
  obs[6 + 2 * no] = (float)(c * (real)m->cassie_target[0] + sn * (real)m->cassie_target[1]);
  obs[6 + 2 * no + 1] = (float)(-sn * (real)m->cassie_target[0] + c * (real)m->cassie_target[1]);
}
/* CassieMoccaEnv.get_obs (:607-627) + phases (:636-642) + the mirrored variant (:657-660): 42 floats */
static void cassie_mocap_obs(Oracle *o, const Dyn *s, const Task *tk, const float *rs, real phase_l, float *obs) {
  const MoccaModel *m = &o->m;
  int no = m->n_ordered;
  real v[42];
  real hr = 0.5 * o->body_rpy[0], hp = 0.5 * o->body_rpy[1], hy = 0.5 * o->body_rpy[2];
  real cr = cos(hr), sr = sin(hr), cp = cos(hp), sp = sin(hp), cy = cos(hy), sy = sin(hy);
  /* pybullet.getQuaternionFromEuler(body_rpy), x y z w  [UNVERIFIED-BULLET: standard ZYX composition] */
  real qx = sr * cp * cy - cr * sp * sy, qy = cr * sp * cy + sr * cp * sy, qz = cr * cp * sy - sr * sp * cy, qw = cr * cp * cy + sr * sp * sy;
  v[0] = s->pos[1]; v[1] = s->pos[2];
  v[2] = qw; v[3] = qx; v[4] = qy; v[5] = qz;
  for (int k = 0; k < no; ++k) { v[6 + k] = cassie_rad(m, k, rs[6 + k]); v[26 + k] = tk->jvel[k]; }
  for (int k = 0; k < 3; ++k) { v[20 + k] = o->body_vel[k]; v[23 + k] = s->omg[k]; }
  v[40] = phase_l;
  v[41] = fmod(phase_l + (real)0.5, (real)1);
  if (m->cassie_mode == MOCCA_CASSIE_PHASE_MIRROR && phase_l > (real)0.5) {
    /* obs[left + right] = obs[right + left]; obs[neg + sideneg] *= -1  (index lists :555-571,633-634,648-655) */
    static const int left[15] = {6, 7, 8, 9, 10, 11, 12, 26, 27, 28, 29, 30, 31, 32, 40};
    static const int right[15] = {13, 14, 15, 16, 17, 18, 19, 33, 34, 35, 36, 37, 38, 39, 41};
    static const int neg[10] = {0, 3, 5, 21, 23, 25, 6, 7, 26, 27};
    for (int k = 0; k < 15; ++k) { real tmp = v[left[k]]; v[left[k]] = v[right[k]]; v[right[k]] = tmp; }
    for (int k = 0; k < 10; ++k) v[neg[k]] = -v[neg[k]];
  }
  for (int i = 0; i < 42; ++i) obs[i] = (float)v[i];
}
/* CassieMocapRewEnv.compute_rewards (:495-531): sum of the six weighted terms */
static real cassie_mocap_reward(Oracle *o, const Dyn *s, const Task *tk, const float *rs, int frame) {
  const MoccaModel *m = &o->m;
  const float *fr = o->traj + (size_t)frame * MOCCA_TRAJ_STRIDE;
  int npow = m->n_ctrl - 2;
  real jp = 0, jv = 0;
  for (int k = 0; k < npow; ++k) { /* [powered_joint_inds] */
    int oi = m->ctrl_oidx[k];
    real dj = (real)fr[oi] - cassie_rad(m, oi, rs[6 + oi]), dv = (real)fr[14 + oi] - tk->jvel[oi];
    jp += dj * dj; jv += dv * dv;
  }
  real ve = o->body_vel[0] - (real)m->mocap_speed;
  real orient = o->body_rpy[0] * o->body_rpy[0] + o->body_rpy[1] * o->body_rpy[1] + o->body_rpy[2] * o->body_rpy[2];
  real ang = s->omg[0] * s->omg[0] + s->omg[1] * s->omg[1] + s->omg[2] * s->omg[2];
  real cy_ = s->pos[1] - (real)m->init_pos[1], cz_ = s->pos[2] - (real)m->init_pos[2]; /* base_position[1:], :515 */
  return (real)m->mocap_w[0] * exp(-4 * ve * ve) + (real)m->mocap_w[1] * exp(-4 * sqrt(jp)) + (real)m->mocap_w[2] * exp((real)-0.4 * sqrt(jv)) +
         (real)m->mocap_w[3] * exp(-4 * orient) + (real)m->mocap_w[4] * exp(-4 * ang) + (real)m->mocap_w[5] * exp(-4 * (cy_ * cy_ + cz_ * cz_));
}
static real cassie_potential(const Oracle *o, const Dyn *s) { /* calc_potential :348-354 */
  real dx = (real)o->m.cassie_target[0] - s->pos[0], dy = (real)o->m.cassie_target[1] - s->pos[1];
  return -sqrt(dx * dx + dy * dy) / (real)o->m.control_dt;
}
/* CassieEnv.reset :362-378 (nominal pose, at rest); CassieMoccaEnv.reset :585-599 (istep = np_random.randint(0, 10000), kept
 * under rsi; joints, joint speeds and rod angles of the motion at mocap_time(); base at initial_velocity :552) */
static void cassie_reset(Oracle *o, int env, float *obs) {
  const MoccaModel *m = &o->m;
  Dyn *s = &o->dyn[env];
  Task *tk = &o->task[env];
  int ep = tk->episode + 1;
  memset(tk, 0, sizeof(*tk));
  tk->episode = ep; tk->applied_gain = 1;
  for (int b = 1; b <= m->n_joints; ++b) { s->q[b] = m->init_q[b]; s->qd[b] = 0; }
  real phase = 0;
  if (m->cassie_mode != MOCCA_CASSIE_PLAIN) {
    float u = (float)draw_uniform(o, env, tk);
    int is = (int)(u * 10000.0f);
    is = is > 9999 ? 9999 : is;
    tk->istep = m->cassie_rsi ? is : 0;
    const float *fr = o->traj + (size_t)traj_frame(o, tk->istep, &phase) * MOCCA_TRAJ_STRIDE;
    for (int k = 0; k < m->n_ordered; ++k) {
      int b = m->ordered_body[k];
      s->q[b] = fr[k]; s->qd[b] = fr[14 + k]; tk->jvel[k] = fr[14 + k];
    }
    for (int k = 0; k < 4; ++k) { s->q[m->rod_body[k]] = fr[28 + k]; s->qd[m->rod_body[k]] = 0; }
  }
  for (int k = 0; k < 3; ++k) { s->pos[k] = m->init_pos[k]; s->vel[k] = m->init_vel[k]; s->omg[k] = 0; }
  for (int k = 0; k < 4; ++k) s->quat[k] = m->init_quat[k];
  for (int k = 0; k < MOCCA_MAX_SLOTS; ++k) s->warm[k] = 0;
  tk->initial_z = s->pos[2];
  kinematics(m, s, &o->wk);
  float rs[6 + 2 * MOCCA_MAX_CTRL];
  cassie_state(o, s, tk, rs);
  if (m->cassie_mode == MOCCA_CASSIE_PLAIN) cassie_obs(o, s, rs, obs);
  else cassie_mocap_obs(o, s, tk, rs, phase, obs);
  tk->linear_potential = cassie_potential(o, s);
}
static void cassie_step(Oracle *o, int env, const float *act, float *obs, float *rew, uint8_t *done, int32_t *info, int physics) {
  const MoccaModel *m = &o->m;
  Dyn *s = &o->dyn[env];
  Task *tk = &o->task[env];
  Work *w = &o->wk;
  int nc = m->n_ctrl, no = m->n_ordered, npow = nc - 2, mode = m->cassie_mode;
  real target[MOCCA_MAX_CTRL], tau[MB], q0[MOCCA_MAX_CTRL];
  const float *f0 = mode != MOCCA_CASSIE_PLAIN ? o->traj + (size_t)traj_frame(o, tk->istep, NULL) * MOCCA_TRAJ_STRIDE : NULL;
  for (int k = 0; k < nc; ++k) { /* :434-443; base_angles() of the mocap envs = the motion at mocap_time() (:601-602) */
    real base = (real)m->ctrl_base[k];
    if (f0) base = (k < npow && m->residual_control) ? (real)f0[m->ctrl_oidx[k]] : 0;
    target[k] = base + (k < npow ? (real)act[k] : 0);
  }
  /* jpos = robot.rad_joint_angles (:447,467): to_radians of the float32 normalised angles */
  for (int k = 0; k < no; ++k) q0[k] = cassie_rad(m, k, cassie_nrm(m, k, s->q[m->ordered_body[k]]));
  if (physics) dbg_step_start(o, env);
  for (int it = 0; physics && it < m->n_llc; ++it) { /* :450-459 */
    for (int k = 0; k < no; ++k)
      tk->jvel[k] = (1 - (real)m->jvel_alpha) * tk->jvel[k] + (real)m->jvel_alpha * (real)(float)s->qd[m->ordered_body[k]];
    for (int b = 0; b <= m->n_joints; ++b) tau[b] = 0;
    for (int k = 0; k < nc; ++k) { /* pd_control :380-393, apply_action :225-230 */
      int b = m->ctrl_body[k], oi = m->ctrl_oidx[k];
      real perr = target[k] - (real)(float)s->q[b];
      real verr = 0 - tk->jvel[oi];
      verr = verr < -5 ? -5 : (verr > 5 ? 5 : verr);
      real t = (real)m->ctrl_kp[k] * perr + (real)m->ctrl_kd[k] * verr, lim = m->torque_limit[b];
      tau[b] = t < -lim ? -lim : (t > lim ? lim : t);
    }
    substep(o, s, tk, &o->ter[env], tau, w);
    dbg_commit(o, env, w);
  }
  tk->istep += m->n_llc; /* pd_control counts every low-level iteration (:381) */
  for (int k = 0; k < no; ++k) /* :467-468 */
    tk->jvel[k] = (cassie_rad(m, k, cassie_nrm(m, k, s->q[m->ordered_body[k]])) - q0[k]) / (real)m->control_dt;
  tk->t += 1;
  kinematics(m, s, w);
  float rs[6 + 2 * MOCCA_MAX_CTRL];
  real height = cassie_state(o, s, tk, rs);
  int finite = 1;
  for (int i = 0; i < 6 + 2 * no; ++i) if (!isfinite(rs[i])) finite = 0;
  real old = tk->linear_potential;
  tk->linear_potential = cassie_potential(o, s);
  real alive = height > (real)m->alive_height ? 2 : -1; /* :401-414 */
  if (!finite || alive < 0) tk->done = 1;
  if (mode == MOCCA_CASSIE_PLAIN) {
    cassie_obs(o, s, rs, obs);
    *rew = (float)(alive + (tk->linear_potential - old));
  } else { /* CassieMocapRewEnv.compute_rewards replaces the reward and keeps `dead` (:495-531) */
    real phase;
    int f1 = traj_frame(o, tk->istep, &phase);
    *rew = (float)cassie_mocap_reward(o, s, tk, rs, f1);
    cassie_mocap_obs(o, s, tk, rs, phase, obs);
  }
  *info = 0;
  int timeout = tk->t >= m->max_episode_steps;
  *done = (uint8_t)((tk->done ? 1 : 0) | (timeout ? 2 : 0));
  if (o->auto_reset && (*done)) cassie_reset(o, env, obs);
}

/* reset one env.  The pose randomisation follows robots.py:179-210 with Philox draws. */
static void reset_env(Oracle *o, int env, float *obs) {
  if (o->task_id == MOCCA_TASK_CASSIE) { cassie_reset(o, env, obs); return; }
  const MoccaModel *m = &o->m;
  Dyn *s = &o->dyn[env];
  Task *tk = &o->task[env];
  Terrain *tr = &o->ter[env];
  int nj = m->n_joints;
  int keep_cur = tk->curriculum;
  int ep = tk->episode + 1;
  /* Walker3DStepperEnv.reset (env_locomotion.py:484-499): calc_feet_state() runs right after robot.reset(), on the contact manifolds of the
   * episode that just ended (Bullet has not stepped since) and with the OLD next_step_index -- MOCCA_TASKF_STALE_RESET_CONTACTS */
  real stale_fc[MOCCA_MAX_FEET];
  for (int k = 0; k < MOCCA_MAX_FEET; ++k) stale_fc[k] = tk->feet_contact[k];
  int stale_nsi = tk->next_step_index, stale_cover = tk->cover;
  /* the random-reward weights are drawn by step() (env_locomotion.py:533-547), not by reset(): a reset leaves the last step's weights in
   * the record, as the kernel's reset does (it rebuilds the task registers only) */
  real keep_rw[8];
  memcpy(keep_rw, tk->rw, sizeof(keep_rw));
  memset(tk, 0, sizeof(*tk));
  tk->episode = ep; tk->curriculum = keep_cur;
  memcpy(tk->rw, keep_rw, sizeof(keep_rw));

  tk->applied_gain = 1;
  if (o->task_id == MOCCA_TASK_WALKER3D_CUSTOM) {
    randomize_target(o, env, tk); /* draws 0..2 */
    tk->walk_target[0] = tk->dist * cos(tk->angle);
    tk->walk_target[1] = tk->dist * sin(tk->angle);
    tk->walk_target[2] = 1;
  } else if (o->task_id == MOCCA_TASK_WALKER3D_PLANNER) {
    /* the target is drawn AFTER robot.reset (env_locomotion.py:1052-1062): below */
  } else {
    tk->applied_gain = DEC(m->gain_cur[0]) + (DEC(m->gain_cur[1]) - DEC(m->gain_cur[0])) * tk->curriculum / 9; /* applied_gain_curriculum[curriculum], :369,489 */
  }
  /* robot.reset */
  real u = draw_uniform(o, env, tk);
  tk->mirrored = u < (real)0.5;
  real base[MB];
  for (int b = 1; b <= nj; ++b) base[b] = m->init_q[b];
  if (tk->mirrored) { /* robots.py:182-188 */
    for (int k = 0; k < m->n_mirror_side; ++k) {
      int r = m->mirror_right[k] + 1, l = m->mirror_left[k] + 1;
      real t = base[r]; base[r] = base[l]; base[l] = t;
    }
    for (int k = 0; k < m->n_mirror_neg; ++k) base[m->mirror_neg[k] + 1] *= -1;
  }
  real dsv[MB];
  for (int b = 1; b <= nj; ++b) /* the deviations are drawn only inside `if random_pose` (robots.py:190-192) */
    dsv[b] = o->random_pose ? (real)-0.1 + (real)0.2 * draw_uniform(o, env, tk) : 0;
  for (int b = 1; b <= nj; ++b) {
    s->q[b] = base[b];
    if (o->random_pose) { /* robots.py:190-194: deviation + normalise + clip(+-0.95) only inside `if random_pose` */
      real wt = (real)(float)(m->jhi[b] - m->jlo[b]), bs = m->jlo[b];
      real ps = 2 * (base[b] + dsv[b] - bs) / wt - 1;
      ps = ps < (real)-0.95 ? (real)-0.95 : (ps > (real)0.95 ? (real)0.95 : ps);
      s->q[b] = wt * (ps + 1) / 2 + bs;
    }
    s->qd[b] = 0;
  }
  for (int k = 0; k < 3; ++k) { s->pos[k] = m->init_pos[k]; s->vel[k] = m->init_vel[k]; s->omg[k] = 0; } /* robot_init_velocity, :92,493 */
  for (int k = 0; k < 4; ++k) s->quat[k] = m->init_quat[k];
  for (int k = 0; k < MOCCA_MAX_SLOTS; ++k) s->warm[k] = 0;
  kinematics(m, s, &o->wk);
  int jal; float spd[MB];
  calc_robot_state(o, s, tk, obs, &jal, spd);
  int nb = 6 + 2 * nj + m->n_feet;
  if (o->task_id == MOCCA_TASK_WALKER3D_PLANNER) { /* Walker3DPlannerEnv.reset, :1060-1073 */
    real ux = draw_uniform(o, env, tk), uy = draw_uniform(o, env, tk), R = m->target_range;
    tk->walk_target[0] = -R + 2 * R * ux;
    tk->walk_target[1] = -R + 2 * R * uy;
    tk->walk_target[2] = (real)(float)hf_height_at(o, tk->walk_target[0], tk->walk_target[1]);
    for (int k = 0; k < 3; ++k) tk->walk_target[k] = (real)(float)tk->walk_target[k]; /* np.array(..., dtype=np.float32), :1062 */
    real dist, ang;
    calc_potential(o, s, tk, &dist, &ang);
    softsign_tail(dist, ang, obs + nb);
  } else if (o->task_id == MOCCA_TASK_WALKER3D_CUSTOM) {
    real dist, ang;
    calc_potential(o, s, tk, &dist, &ang);
    softsign_tail(dist, ang, obs + nb);
    if (m->task_flags & MOCCA_TASKF_RESET_TAIL_ZERO) { obs[nb] = 0; obs[nb + 1] = 0; } /* Walker2DCustomEnv.reset, :299-300 */
  } else {
    /* env_locomotion.py:481-513: robot.reset()'s observation (above) carries feet_contact = 0 (robots.py:197-200); calc_feet_state() then
     * runs on the manifolds of the episode before -- the first step's observation shows its flags (:525) -- or, flag cleared, finds nothing */
    if (m->task_flags & MOCCA_TASKF_STALE_RESET_CONTACTS) {
      int reached = 0;
      for (int k = 0; k < m->n_feet; ++k) {
        tk->feet_contact[k] = stale_fc[k];                                         /* robot.feet_contact[:] = info[:, 0], :656 */
        reached |= (stale_cover >> (4 * k + stale_nsi % m->n_planks)) & 1;
      }
      if (reached) tk->target_reached_count = 1;                                   /* += 1 from 0 (:484,661); below 2: nothing advances */
    }
    generate_step_placements(o, env, tk, tr);
    for (int k = 0; k < MOCCA_MAX_PLANKS; ++k) tr->plank_info[k] = k;
    tk->next_step_index = m->lookbehind; /* :499 */
    delta_to_k_targets(o, s, tk, tr, obs + nb);
    real dist, ang;
    calc_potential(o, s, tk, &dist, &ang);
  }
  tk->prev_body_x = s->pos[0];
}

static void step_env(Oracle *o, int env, const float *act, float *obs, float *rew, uint8_t *done, int32_t *info,
                     const int32_t *ext_touch, const int32_t *ext_target, const int32_t *ext_body) {
  if (o->task_id == MOCCA_TASK_CASSIE) { cassie_step(o, env, act, obs, rew, done, info, 1); return; }
  const MoccaModel *m = &o->m;
  Dyn *s = &o->dyn[env];
  Task *tk = &o->task[env];
  Terrain *tr = &o->ter[env];
  Work *w = &o->wk;
  int nj = m->n_joints, nb = 6 + 2 * nj + m->n_feet;
  real tau[MB];
  tau[0] = 0;
  for (int b = 1; b <= nj; ++b) { /* robots.py:31-40 */
    real a = act[b - 1];
    a = a < -1 ? -1 : (a > 1 ? 1 : a);
    tau[b] = (real)m->gain[b] * tk->applied_gain * a;
  }
  int touch[MOCCA_MAX_FEET] = {0}, target[MOCCA_MAX_FEET] = {0}, body_touch = 0, cover = 0;
  if (!ext_touch) {
    dbg_step_start(o, env);
    for (int k = 0; k < m->n_substeps; ++k) { substep(o, s, tk, tr, tau, w); dbg_commit(o, env, w); }
    /* contact queries after stepSimulation see the manifolds of the LAST substep's collision pass */
    for (int k = 0; k < m->n_feet; ++k) { touch[k] = w->foot_touch[k]; target[k] = w->foot_target[k]; }
    body_touch = w->body_touch;
    cover = w->cover;
  } else {
    /* task-only step (golden tests): the caller injected the post-physics state and the contacts; per foot: 1 = on the cover of the target
     * plank (plank next_step_index mod n_planks at the step's start), 2 = on the cover of the plank after it */
    int npl = o->task_id == MOCCA_TASK_WALKER3D_STEPPER ? m->n_planks : 1;
    for (int k = 0; k < m->n_feet; ++k) {
      touch[k] = ext_touch[k]; target[k] = ext_target[k] == 1;
      if (ext_target[k] == 1 || ext_target[k] == 2) cover |= 1 << (4 * k + (tk->next_step_index + ext_target[k] - 1) % npl);
    }
    body_touch = ext_body ? *ext_body : 0;
  }
  tk->t += 1;
  kinematics(m, s, w);
  int jal; float spd[MB];
  real dist, ang, progress, posture = 0, energy, joints, tall, target_bonus = 0, step_bonus = 0;
  if (o->task_id == MOCCA_TASK_WALKER3D_PLANNER) {
    /* Walker3DPlannerEnv.step, env_locomotion.py:1075-1128.  calc_state() is called without contact ids: feet_contact keeps the
     * zeros of robot.reset.  The reward's second term, log(max(1, base_value)) / 3, is the external base controller's value estimate:
     * the caller adds it (mocca_envs_amd/envs.py); here reward = progress. */
    for (int k = 0; k < m->n_feet; ++k) tk->feet_contact[k] = 0;
    calc_robot_state(o, s, tk, obs, &jal, spd);
    real old = tk->linear_potential;
    calc_potential(o, s, tk, &dist, &ang);
    progress = tk->linear_potential - old;
    /* done = done or relative torso height < termination_height or z < -5 or the torso link touches anything (:1103-1111);
     * NaN comparisons are False, as in the reference */
    if (obs[0] < m->termination_height || s->pos[2] < (real)m->fall_z || body_touch) tk->done = 1;
    *rew = (float)progress;
    softsign_tail(dist, ang, obs + nb);
    *info = 0;
  } else if (o->task_id == MOCCA_TASK_WALKER3D_CUSTOM) {
    if (o->eval_mode) { tk->walk_target[0] = tk->prev_body_x + 4; tk->walk_target[1] = 0; tk->walk_target[2] = 1; } /* :115-116 */
    for (int k = 0; k < m->n_feet; ++k) tk->feet_contact[k] = touch[k]; /* robots.py:74-86 */
    calc_robot_state(o, s, tk, obs, &jal, spd);
    int finite = 1;
    for (int i = 0; i < nb; ++i) if (!isfinite(obs[i])) finite = 0;
    if (!finite) tk->done = 1; /* :205-207 */
    real old = tk->linear_potential;
    calc_potential(o, s, tk, &dist, &ang);
    progress = tk->linear_potential - old;
    real pitch = o->body_rpy[1], roll = o->body_rpy[0];
    if (!((real)-0.2 < pitch && pitch < (real)0.4)) posture = fabs(pitch); /* :178-183 */
    if (!((real)-0.4 < roll && roll < (real)0.4)) posture += fabs(roll);
    real e1 = 0, e2 = 0;
    for (int j = 0; j < nj; ++j) { e1 += fabs((real)act[j] * (real)spd[j]); e2 += (real)act[j] * (real)act[j]; }
    energy = (real)m->electricity_cost * (e1 / nj) + (real)m->stall_torque_cost * (e2 / nj);
    joints = (real)m->joints_at_limit_cost * jal;
    tall = obs[0] > m->termination_height ? 2 : -1;
    if (tall < 0) tk->done = 1;
    if (m->task_flags & MOCCA_TASKF_BODY_CONTACT) { /* LaikagoCustomEnv.calc_base_reward, :877-890 */
      tall = 0;
      if (body_touch) { tall = -1; tk->done = 1; }
    }
    if (dist < (real)0.15) { tk->close_count += 1; target_bonus = 2; } /* :198-202 */
    if (tk->close_count >= tk->stop_frames) { /* :214-222 */
      tk->close_count = 0;
      randomize_target(o, env, tk);
      tk->walk_target[0] += tk->dist * cos(tk->angle);
      tk->walk_target[1] += tk->dist * sin(tk->angle);
      calc_potential(o, s, tk, &dist, &ang);
    }
    *rew = (float)(progress + target_bonus - energy + tall - posture - joints); /* :121-122 */
    softsign_tail(dist, ang, obs + nb);
    if (m->task_flags & MOCCA_TASKF_NEVER_DONE) tk->done = 0; /* Walker2DCustomEnv.step, :302-309 */
    *info = 0;
  } else {
    /* env_locomotion.py:515-568 */
    tk->set_stop_on_next_step = (tk->next_step_index == 6 || tk->next_step_index == 7 ||
                                 tk->next_step_index == 13 || tk->next_step_index == 14); /* :522 */
    calc_robot_state(o, s, tk, obs, &jal, spd); /* previous step's feet_contact, :525 */
    int finite = 1;
    for (int i = 0; i < nb; ++i) if (!isfinite(obs[i])) finite = 0;
    if (!finite) tk->done = 1;
    int cur_step_index = tk->next_step_index;
    /* calc_feet_state :632-674 */
    real fd[MOCCA_MAX_FEET];
    int target_reached = 0;
    for (int k = 0; k < m->n_feet; ++k) {
      real dx = o->feet_xyz[k][0] - tr->terrain[tk->next_step_index][0];
      real dy = o->feet_xyz[k][1] - tr->terrain[tk->next_step_index][1];
      fd[k] = sqrt(dx * dx + dy * dy);
      tk->feet_contact[k] = touch[k];
      if (target[k]) target_reached = 1;
    }
    tk->cover = cover; /* what a reset() right after this step would still read */
    if (target_reached) {
      tk->target_reached_count += 1;
      if (tk->target_reached_count > 120) { tk->stop_on_next_step = 0; tk->set_stop_on_next_step = 0; }
      if (tk->target_reached_count >= 2) {
        if (!tk->stop_on_next_step) {
          tk->next_step_index += 1;
          tk->target_reached_count = 0;
          if (tk->next_step_index >= m->n_planks) { /* update_steps :472-479 */
            int oldest = tk->next_step_index % m->n_planks;
            int nx = tk->next_step_index < MOCCA_MAX_TERRAIN_STEPS - 1 ? tk->next_step_index : MOCCA_MAX_TERRAIN_STEPS - 1;
            tr->plank_info[oldest] = nx;
          }
        }
        tk->stop_on_next_step = tk->set_stop_on_next_step;
      }
      if (tk->next_step_index >= MOCCA_MAX_TERRAIN_STEPS) tk->next_step_index -= 1;
    }
    /* calc_base_reward :598-630 */
    real old = tk->linear_potential;
    calc_potential(o, s, tk, &dist, &ang);
    progress = tk->linear_potential - old;
    real pitch = o->body_rpy[1], roll = o->body_rpy[0];
    real e1 = 0, e2 = 0;
    for (int j = 0; j < nj; ++j) { e1 += fabs((real)act[j] * (real)spd[j]); e2 += (real)act[j] * (real)act[j]; }
    energy = (real)m->electricity_cost * (e1 / nj) + (real)m->stall_torque_cost * (e2 / nj);
    joints = (real)m->joints_at_limit_cost * jal;
    if (!(m->task_flags & MOCCA_TASKF_QUADRUPED_STEPPER)) {
      if (!((real)-0.2 < pitch && pitch < (real)0.4)) posture = fabs(pitch);
      if (!((real)-0.4 < roll && roll < (real)0.4)) posture += fabs(roll);
      real term_h = DEC(m->term_height_cur[0]) + (DEC(m->term_height_cur[1]) - DEC(m->term_height_cur[0])) * tk->curriculum / 9; /* :368,628 */
      tall = obs[0] > term_h ? 2 : -1;
      if (tall < 0) tk->done = 1;
    } else {
      /* LaikagoStepperEnv.calc_base_reward, :928-979: posture from the hip_x / hip_y / knee angles (degrees, float32 joint
       * angles as robot.joint_angles holds them), progress x 2, posture x 0.2, time-based early termination REPLACES done */
      const real R2D = (real)(180.0 / 3.14159265358979323846), D2R = (real)(3.14159265358979323846 / 180.0);
      for (int j = 0; j < nj; ++j) {
        real a = (real)(float)s->q[1 + j] * R2D, lo_ = j % 3 == 0 ? -25 : (j % 3 == 1 ? -35 : -75), hi_ = j % 3 == 0 ? 25 : (j % 3 == 1 ? 35 : -15);
        if (!(lo_ < a && a < hi_)) posture += fabs(a * D2R);
      }
      if (!(-25 < pitch * R2D && pitch * R2D < 25)) posture += fabs(pitch);
      progress *= 2;
      posture *= (real)0.2;
      tall = 2;
      tk->done = (tk->t > 240 && tk->next_step_index <= 4);
      if (body_touch) { tall = -1; tk->done = 1; }
    }
    /* calc_step_reward :676-693 */
    int last = MOCCA_MAX_TERRAIN_STEPS - 1;
    if (target_reached && tk->target_reached_count == 1 && tk->next_step_index != last) {
      real dmin = fd[0];
      for (int k = 1; k < m->n_feet; ++k) if (fd[k] < dmin) dmin = fd[k];
      step_bonus = 50 * pow((real)2.718, -pow(dmin, (real)m->step_bonus_smoothness) / (real)0.25);
    }
    if ((tk->next_step_index == last || tk->stop_on_next_step) && dist < (real)0.15) target_bonus = 2;
    delta_to_k_targets(o, s, tk, tr, obs + nb);
    if (cur_step_index != tk->next_step_index) calc_potential(o, s, tk, &dist, &ang);
    if (!o->random_reward) {
      *rew = (float)(progress - energy + step_bonus + target_bonus + tall - posture - joints); /* :528-531 */
    } else { /* :533-547: np.dot(np_random.uniform(0.8, 1.2, 8), terms) */
      if (o->random_reward == 1)
        for (int k = 0; k < 8; ++k) tk->rw[k] = (real)0.8 + (real)0.4 * draw_uniform(o, env, tk);
      const real terms[8] = {progress, -energy, step_bonus, target_bonus, 0, tall, -posture, -joints};
      real acc = 0;
      for (int k = 0; k < 8; ++k) acc += tk->rw[k] * terms[k];
      *rew = (float)acc;
    }
    *info = tk->next_step_index;
  }
  tk->prev_body_x = s->pos[0];
  int timeout = tk->t >= m->max_episode_steps;
  *done = (uint8_t)((tk->done ? 1 : 0) | (timeout ? 2 : 0));
  if (o->auto_reset && (*done)) reset_env(o, env, obs);
}

/* ------------------------------------------------------------------ */
/* C API (mirrors include/mocca.h on host pointers)                    */
/* ------------------------------------------------------------------ */
API int orc_real_bytes(void) { return (int)sizeof(real); }
API int orc_model_sizeof(void) { return (int)sizeof(MoccaModel); }

API void *orc_create(const void *blob, int nbytes, int task_id, int n_envs) {
  if (nbytes != (int)sizeof(MoccaModel)) return NULL;
  Oracle *o = (Oracle *)calloc(1, sizeof(Oracle));
  memcpy(&o->m, blob, sizeof(MoccaModel));
  if (o->m.magic != MOCCA_MODEL_MAGIC || o->m.version != MOCCA_MODEL_VERSION || o->m.max_contacts > MAX_CONTACTS ||
      o->m.max_rows > MAX_ROWS) { free(o); return NULL; }
  o->task_id = task_id; o->n_envs = n_envs; o->random_pose = 1;
  o->dyn = (Dyn *)calloc(n_envs, sizeof(Dyn));
  o->task = (Task *)calloc(n_envs, sizeof(Task));
  o->ter = (Terrain *)calloc(n_envs, sizeof(Terrain));
  o->dbg = (int32_t *)calloc((size_t)n_envs * DBG_WORDS, sizeof(int32_t));
  for (int e = 0; e < n_envs; ++e) { o->dyn[e].quat[3] = 1; o->task[e].applied_gain = 1; o->task[e].episode = -1; }
  return o;
}
API void orc_destroy(void *h) {
  Oracle *o = (Oracle *)h;
  if (!o) return;
  free(o->dyn); free(o->task); free(o->ter); free(o->dbg); free(o->traj); free(o->hf); free(o);
}
/* the reference motion of the Cassie mocap / phase envs (mocca_set_trajectory of include/mocca.h): copied */
API int orc_set_trajectory(void *h, const float *table, int n_frames, double max_time, double control_step) {
  Oracle *o = (Oracle *)h;
  if (!o || !table || n_frames <= 0 || !(max_time > 0) || !(control_step > 0)) return -1;
  free(o->traj);
  o->traj = (float *)malloc((size_t)n_frames * MOCCA_TRAJ_STRIDE * sizeof(float));
  memcpy(o->traj, table, (size_t)n_frames * MOCCA_TRAJ_STRIDE * sizeof(float));
  o->traj_n = n_frames; o->traj_tmax = max_time; o->traj_cstep = control_step;
  return 0;
}
/* the planner envs' terrain (mocca_set_heightfield of include/mocca.h): copied */
API int orc_set_heightfield(void *h, const float *data, int rows, int cols, double scale) {
  Oracle *o = (Oracle *)h;
  if (!o || !data || rows < 2 || cols < 2 || !(scale > 0)) return -1;
  free(o->hf);
  o->hf = (float *)malloc((size_t)rows * cols * sizeof(float));
  memcpy(o->hf, data, (size_t)rows * cols * sizeof(float));
  o->hf_rows = rows; o->hf_cols = cols; o->hf_scale = scale;
  return 0;
}
/* probe for the tests: gap and normal of a sphere (world centre, radius) against the attached height field; get_height_at */
API double orc_heightfield_probe(void *h, const double *c, double rad, double margin, double *n_out) {
  Oracle *o = (Oracle *)h;
  real C[3] = {(real)c[0], (real)c[1], (real)c[2]}, n[3];
  real g = sphere_heightfield(o, C, (real)rad, hf_window(o, rad + margin), n);
  for (int k = 0; k < 3; ++k) n_out[k] = n[k];
  return g;
}
API double orc_height_at(void *h, double x, double y) { return hf_height_at((Oracle *)h, (real)x, (real)y); }
API int orc_obs_dim(void *h) { return obs_dim((Oracle *)h); }
API int orc_act_dim(void *h) { Oracle *o = (Oracle *)h; return o->task_id == MOCCA_TASK_CASSIE ? o->m.n_ctrl - 2 : o->m.n_joints; }
API int orc_state_dim(void *h) { Oracle *o = (Oracle *)h; return MOCCA_STATE_DIM(o->m.n_joints, o->m.n_slots); }

enum { PARAM_AUTO_RESET = 0, PARAM_EVAL_MODE = 1, PARAM_CURRICULUM = 2, PARAM_RANDOM_POSE = 3, PARAM_RANDOM_REWARD = 8 /* ids of include/mocca.h */ };
API void orc_set_param(void *h, int id, double v) {
  Oracle *o = (Oracle *)h;
  if (id == PARAM_AUTO_RESET) o->auto_reset = v != 0;
  else if (id == PARAM_EVAL_MODE) o->eval_mode = v != 0;
  else if (id == PARAM_CURRICULUM) for (int e = 0; e < o->n_envs; ++e) o->task[e].curriculum = (int)v;
  else if (id == PARAM_RANDOM_POSE) o->random_pose = v != 0;
  else if (id == PARAM_RANDOM_REWARD) o->random_reward = (int)v;
}

API void orc_reset(void *h, const uint8_t *mask, uint64_t seed, float *obs) {
  Oracle *o = (Oracle *)h;
  int od = obs_dim(o);
  o->seed = seed;
  for (int e = 0; e < o->n_envs; ++e)
    if (!mask || mask[e]) reset_env(o, e, obs + (size_t)e * od);
}
API void orc_step(void *h, const float *act, float *obs, float *rew, uint8_t *done, int32_t *info) {
  Oracle *o = (Oracle *)h;
  int od = obs_dim(o), nj = o->task_id == MOCCA_TASK_CASSIE ? o->m.n_ctrl - 2 : o->m.n_joints;
  for (int e = 0; e < o->n_envs; ++e) {
    int32_t inf = 0;
    step_env(o, e, act + (size_t)e * nj, obs + (size_t)e * od, rew + e, done + e, &inf, NULL, NULL, NULL);
    if (info) info[e] = inf;
  }
}
/* `steps` env.steps in ONE call, actions from a looped tape [tape_len][N][act_dim]; outputs discarded.  bench.py's all-cores CPU baseline:
 * one call per host thread, so the threads never meet at the interpreter lock between steps. */
API void orc_rollout(void *h, const float *tape, int tape_len, int steps) {
  Oracle *o = (Oracle *)h;
  int od = obs_dim(o), nj = o->task_id == MOCCA_TASK_CASSIE ? o->m.n_ctrl - 2 : o->m.n_joints;
  float *obs = (float *)malloc(sizeof(float) * (size_t)o->n_envs * od), *rew = (float *)malloc(sizeof(float) * o->n_envs);
  uint8_t *done = (uint8_t *)malloc(o->n_envs);
  if (obs && rew && done)
    for (int k = 0; k < steps; ++k) orc_step(h, tape + (size_t)(k % tape_len) * o->n_envs * nj, obs, rew, done, NULL);
  free(obs); free(rew); free(done);
}
/* task logic only: the dynamic state currently stored is taken as the post-stepSimulation state,
 * touch/target [N][2] are the foot contact query results. */
API void orc_task_step(void *h, const float *act, const int32_t *touch, const int32_t *target, float *obs, float *rew,
                       uint8_t *done, int32_t *info) {
  Oracle *o = (Oracle *)h;
  int od = obs_dim(o), nj = o->m.n_joints;
  for (int e = 0; e < o->n_envs; ++e) {
    int32_t inf = 0;
    step_env(o, e, act + (size_t)e * nj, obs + (size_t)e * od, rew + e, done + e, &inf, touch + 2 * e, target + 2 * e, NULL);
    if (info) info[e] = inf;
  }
}
/* the same for any foot count: touch / target are [N][n_feet], body_touch [N] (non-foot link on the ground) or NULL */
API void orc_task_step_feet(void *h, const float *act, const int32_t *touch, const int32_t *target, const int32_t *body_touch,
                            float *obs, float *rew, uint8_t *done, int32_t *info) {
  Oracle *o = (Oracle *)h;
  int od = obs_dim(o), nj = o->m.n_joints, nf = o->m.n_feet;
  for (int e = 0; e < o->n_envs; ++e) {
    int32_t inf = 0;
    step_env(o, e, act + (size_t)e * nj, obs + (size_t)e * od, rew + e, done + e, &inf, touch + nf * e, target + nf * e,
             body_touch ? body_touch + e : NULL);
    if (info) info[e] = inf;
  }
}
API void orc_set_tape(void *h, const double *tape, int n) {
  Oracle *o = (Oracle *)h;
  o->tape = tape; o->tape_n = n; o->tape_pos = 0;
}
/* dynamic state, layout of include/mocca_model.h (doubles so both builds share the binding) */
API void orc_get_state(void *h, double *st) {
  Oracle *o = (Oracle *)h;
  int nj = o->m.n_joints, ns = o->m.n_slots, S = MOCCA_STATE_DIM(nj, ns);
  for (int e = 0; e < o->n_envs; ++e) {
    const Dyn *s = &o->dyn[e];
    double *p = st + (size_t)e * S;
    for (int k = 0; k < 3; ++k) { p[k] = s->pos[k]; p[7 + k] = s->vel[k]; p[10 + k] = s->omg[k]; }
    for (int k = 0; k < 4; ++k) p[3 + k] = s->quat[k];
    for (int b = 1; b <= nj; ++b) { p[13 + b - 1] = s->q[b]; p[13 + nj + b - 1] = s->qd[b]; }
    for (int k = 0; k < ns; ++k) p[13 + 2 * nj + k] = s->warm[k];
  }
}
API void orc_set_state(void *h, const double *st) {
  Oracle *o = (Oracle *)h;
  int nj = o->m.n_joints, ns = o->m.n_slots, S = MOCCA_STATE_DIM(nj, ns);
  for (int e = 0; e < o->n_envs; ++e) {
    Dyn *s = &o->dyn[e];
    const double *p = st + (size_t)e * S;
    for (int k = 0; k < 3; ++k) { s->pos[k] = (real)p[k]; s->vel[k] = (real)p[7 + k]; s->omg[k] = (real)p[10 + k]; }
    for (int k = 0; k < 4; ++k) s->quat[k] = (real)p[3 + k];
    for (int b = 1; b <= nj; ++b) { s->q[b] = (real)p[13 + b - 1]; s->qd[b] = (real)p[13 + nj + b - 1]; }
    for (int k = 0; k < ns; ++k) s->warm[k] = (real)p[13 + 2 * nj + k];
  }
}
/* task record: MOCCA_TASK_WORDS doubles per env, same word order as include/mocca_model.h */
API void orc_get_task(void *h, double *t) {
  Oracle *o = (Oracle *)h;
  for (int e = 0; e < o->n_envs; ++e) {
    const Task *k = &o->task[e];
    double *p = t + (size_t)e * MOCCA_TASK_WORDS;
    memset(p, 0, MOCCA_TASK_WORDS * sizeof(double));
    for (int j = 0; j < 3; ++j) p[MOCCA_TW_WALK_TARGET_X + j] = k->walk_target[j];
    p[MOCCA_TW_LINEAR_POTENTIAL] = k->linear_potential; p[MOCCA_TW_ANGULAR_POTENTIAL] = k->angular_potential;
    p[MOCCA_TW_CLOSE_COUNT] = k->close_count; p[MOCCA_TW_STOP_FRAMES] = k->stop_frames;
    p[MOCCA_TW_DONE] = k->done; p[MOCCA_TW_T] = k->t; p[MOCCA_TW_EPISODE] = k->episode; p[MOCCA_TW_DRAW] = k->draw;
    p[MOCCA_TW_MIRRORED] = k->mirrored;
    p[MOCCA_TW_FEET_CONTACT_0] = k->feet_contact[0]; p[MOCCA_TW_FEET_CONTACT_1] = k->feet_contact[1];
    p[MOCCA_TW_DIST] = k->dist; p[MOCCA_TW_ANGLE] = k->angle;
    p[MOCCA_TW_NEXT_STEP_INDEX] = k->next_step_index; p[MOCCA_TW_TARGET_REACHED_COUNT] = k->target_reached_count;
    p[MOCCA_TW_STOP_ON_NEXT_STEP] = k->stop_on_next_step; p[MOCCA_TW_SET_STOP_ON_NEXT_STEP] = k->set_stop_on_next_step;
    p[MOCCA_TW_CURRICULUM] = k->curriculum; p[MOCCA_TW_APPLIED_GAIN] = k->applied_gain; p[MOCCA_TW_PREV_BODY_X] = k->prev_body_x;
    for (int j = 0; j < 14; ++j) p[MOCCA_TW_JVEL + j] = k->jvel[j];
    if (o->m.n_feet > 2) { p[MOCCA_TW_FEET_CONTACT_2] = k->feet_contact[2]; p[MOCCA_TW_FEET_CONTACT_3] = k->feet_contact[3]; } /* quadrupeds: words shared with Cassie's jvel */
    p[MOCCA_TW_INITIAL_Z] = k->initial_z; p[MOCCA_TW_ISTEP] = k->istep;
    if (o->task_id == MOCCA_TASK_WALKER3D_STEPPER) {
      for (int j = 0; j < 8; ++j) p[MOCCA_TW_REWARD_WEIGHTS + j] = k->rw[j];
      p[MOCCA_TW_COVER] = k->cover;
    }
  }
}
API void orc_set_task(void *h, const double *t) {
  Oracle *o = (Oracle *)h;
  for (int e = 0; e < o->n_envs; ++e) {
    Task *k = &o->task[e];
    const double *p = t + (size_t)e * MOCCA_TASK_WORDS;
    for (int j = 0; j < 3; ++j) k->walk_target[j] = (real)p[MOCCA_TW_WALK_TARGET_X + j];
    k->linear_potential = (real)p[MOCCA_TW_LINEAR_POTENTIAL]; k->angular_potential = (real)p[MOCCA_TW_ANGULAR_POTENTIAL];
    k->close_count = (int)p[MOCCA_TW_CLOSE_COUNT]; k->stop_frames = (real)p[MOCCA_TW_STOP_FRAMES];
    k->done = (int)p[MOCCA_TW_DONE]; k->t = (int)p[MOCCA_TW_T]; k->episode = (int)p[MOCCA_TW_EPISODE]; k->draw = (int)p[MOCCA_TW_DRAW];
    k->mirrored = (int)p[MOCCA_TW_MIRRORED];
    k->feet_contact[0] = (real)p[MOCCA_TW_FEET_CONTACT_0]; k->feet_contact[1] = (real)p[MOCCA_TW_FEET_CONTACT_1];
    k->dist = (real)p[MOCCA_TW_DIST]; k->angle = (real)p[MOCCA_TW_ANGLE];
    k->next_step_index = (int)p[MOCCA_TW_NEXT_STEP_INDEX]; k->target_reached_count = (int)p[MOCCA_TW_TARGET_REACHED_COUNT];
    k->stop_on_next_step = (int)p[MOCCA_TW_STOP_ON_NEXT_STEP]; k->set_stop_on_next_step = (int)p[MOCCA_TW_SET_STOP_ON_NEXT_STEP];
    k->curriculum = (int)p[MOCCA_TW_CURRICULUM]; k->applied_gain = (real)p[MOCCA_TW_APPLIED_GAIN];
    k->prev_body_x = (real)p[MOCCA_TW_PREV_BODY_X];
    for (int j = 0; j < 14; ++j) k->jvel[j] = (real)p[MOCCA_TW_JVEL + j];
    if (o->m.n_feet > 2) { k->feet_contact[2] = (real)p[MOCCA_TW_FEET_CONTACT_2]; k->feet_contact[3] = (real)p[MOCCA_TW_FEET_CONTACT_3]; }
    k->initial_z = (real)p[MOCCA_TW_INITIAL_Z]; k->istep = (int)p[MOCCA_TW_ISTEP];
    if (o->task_id == MOCCA_TASK_WALKER3D_STEPPER) {
      k->cover = (int)p[MOCCA_TW_COVER];
      for (int j = 0; j < 8; ++j) k->rw[j] = (real)p[MOCCA_TW_REWARD_WEIGHTS + j];
    }
  }
}
API void orc_get_terrain(void *h, double *t) { /* [N][20][6] + plank_info appended per env [3] */
  Oracle *o = (Oracle *)h;
  for (int e = 0; e < o->n_envs; ++e) {
    double *p = t + (size_t)e * (MOCCA_MAX_TERRAIN_STEPS * 6 + MOCCA_MAX_PLANKS);
    for (int i = 0; i < MOCCA_MAX_TERRAIN_STEPS; ++i)
      for (int k = 0; k < 6; ++k) p[6 * i + k] = o->ter[e].terrain[i][k];
    for (int k = 0; k < MOCCA_MAX_PLANKS; ++k) p[MOCCA_MAX_TERRAIN_STEPS * 6 + k] = o->ter[e].plank_info[k];
  }
}
API void orc_set_terrain(void *h, const double *t) {
  Oracle *o = (Oracle *)h;
  for (int e = 0; e < o->n_envs; ++e) {
    const double *p = t + (size_t)e * (MOCCA_MAX_TERRAIN_STEPS * 6 + MOCCA_MAX_PLANKS);
    for (int i = 0; i < MOCCA_MAX_TERRAIN_STEPS; ++i)
      for (int k = 0; k < 6; ++k) o->ter[e].terrain[i][k] = (real)p[6 * i + k];
    for (int k = 0; k < MOCCA_MAX_PLANKS; ++k) o->ter[e].plank_info[k] = (int)p[MOCCA_MAX_TERRAIN_STEPS * 6 + k];
  }
}

/* ---- physics-only probes for the invariant tests ---- */
/* advance env `e` by n substeps with torques tau[nj] (no task logic) */
API void orc_physics_substeps(void *h, int e, const double *tau, int n) {
  Oracle *o = (Oracle *)h;
  real t[MB];
  t[0] = 0;
  for (int b = 1; b <= o->m.n_joints; ++b) t[b] = (real)tau[b - 1];
  for (int k = 0; k < n; ++k) { substep(o, &o->dyn[e], &o->task[e], &o->ter[e], t, &o->wk); dbg_commit(o, e, &o->wk); }
}
/* forward dynamics at the current state: out = [a_base(6, spatial about base origin); qdd(nj)] */
API void orc_forward_dynamics(void *h, int e, const double *tau, int with_bias, double *out) {
  Oracle *o = (Oracle *)h;
  real t[MB];
  t[0] = 0;
  for (int b = 1; b <= o->m.n_joints; ++b) t[b] = (real)tau[b - 1];
  kinematics(&o->m, &o->dyn[e], &o->wk);
  aba(&o->m, &o->dyn[e], t, &o->wk, with_bias);
  for (int k = 0; k < 6; ++k) out[k] = o->wk.acc[0][k];
  for (int b = 1; b <= o->m.n_joints; ++b) out[5 + b] = o->wk.qdd[b];
}
/* out = M^-1 f using the articulated quantities of the last forward dynamics call */
API void orc_minv_apply(void *h, const double *f, double *out) {
  Oracle *o = (Oracle *)h;
  int nd = 6 + o->m.n_joints;
  real ff[NDOF_MAX], oo[NDOF_MAX];
  for (int k = 0; k < nd; ++k) ff[k] = (real)f[k];
  minv_apply(&o->m, &o->wk, ff, oo);
  for (int k = 0; k < nd; ++k) out[k] = oo[k];
}
/* link frames of env e: per body R(9), origin world(3), com world(3) */
API void orc_link_frames(void *h, int e, double *out) {
  Oracle *o = (Oracle *)h;
  kinematics(&o->m, &o->dyn[e], &o->wk);
  for (int b = 0; b < o->m.n_bodies; ++b) {
    double *p = out + 15 * b;
    for (int k = 0; k < 9; ++k) p[k] = o->wk.R[b][k];
    for (int k = 0; k < 3; ++k) { p[9 + k] = o->wk.r[b][k] + o->dyn[e].pos[k]; p[12 + k] = o->wk.comw[b][k] + o->dyn[e].pos[k]; }
  }
}
/* link spatial velocities about the base origin (after kinematics+aba pass 1): [nb][6] */
API void orc_link_velocities(void *h, int e, double *out) {
  Oracle *o = (Oracle *)h;
  real t[MB];
  memset(t, 0, sizeof(t));
  kinematics(&o->m, &o->dyn[e], &o->wk);
  aba(&o->m, &o->dyn[e], t, &o->wk, 1);
  for (int b = 0; b < o->m.n_bodies; ++b)
    for (int k = 0; k < 6; ++k) out[6 * b + k] = o->wk.v[b][k];
}
API void orc_set_precise_gaps(void *h, int bits) { ((Oracle *)h)->wk.precise = bits; } /* experiment, see kinematics_d */
API int orc_last_contacts(void *h, double *out) { /* per contact: a, b, slot, P(3) n(3) depth mu */
  Oracle *o = (Oracle *)h;
  for (int i = 0; i < o->wk.nc; ++i) {
    double *p = out + 11 * i;
    p[0] = o->wk.c_a[i]; p[1] = o->wk.c_b[i]; p[2] = o->wk.c_slot[i];
    for (int k = 0; k < 3; ++k) { p[3 + k] = o->wk.c_P[i][k]; p[6 + k] = o->wk.c_n[i][k]; }
    p[9] = o->wk.c_depth[i]; p[10] = o->wk.c_mu[i];
  }
  return o->wk.nc;
}
API int orc_last_rows(void *h) { return ((Oracle *)h)->wk.nr; }
/* impulses and kinds (0 limit, 1 normal, 2 friction, 3 closure) of the rows of the last substep solved */
API int orc_last_lambda(void *h, double *lam, int32_t *kind) {
  Oracle *o = (Oracle *)h;
  for (int r = 0; r < o->wk.nr; ++r) { lam[r] = o->wk.lam[r]; kind[r] = o->wk.row_kind[r]; }
  return o->wk.nr;
}
/* debug record of every env: [n_envs][MOCCA_DEBUG_WORDS] int32, words as MOCCA_DBG_* (include/mocca.h) */
API void orc_get_debug(void *h, int32_t *out) {
  Oracle *o = (Oracle *)h;
  memcpy(out, o->dbg, (size_t)o->n_envs * DBG_WORDS * sizeof(int32_t));
}
API void orc_clear_debug(void *h) {
  Oracle *o = (Oracle *)h;
  memset(o->dbg, 0, (size_t)o->n_envs * DBG_WORDS * sizeof(int32_t));
}
