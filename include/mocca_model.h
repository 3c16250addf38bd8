/*
 * mocca_model.h -- the flat, versioned model blob shared by the HIP stepper
 * (mocca_envs_amd/csrc), the CPU oracle (oracle/) and the Python model
 * compiler (mocca_envs_amd/model.py mirrors this struct with ctypes).
 *
 * It replaces what the reference obtains from Bullet's importers:
 *   loadMJCF(walker3d.xml)            /root/reference/mocca_envs/robots.py:102
 *   getJointInfo limits [8],[9]       /root/reference/mocca_envs/bullet_utils.py:197-199
 *   power_coef gains                  /root/reference/mocca_envs/robots.py:168,234-256
 *   World.set_physics_parameters      /root/reference/mocca_envs/bullet_utils.py:343-350
 *   StadiumScene ground friction      /root/reference/mocca_envs/bullet_utils.py:361-371
 *
 * Conventions
 *   body 0 is the floating base; body b (1..n_joints) hangs off parent[b] by
 *   one hinge whose value is q[b-1].  Bodies are in topological (DFS) order so
 *   parent[b] < b, and q order equals the reference's `ordered_joints`.
 *   A body frame has its origin at the hinge anchor; jpos/jrot give it in the
 *   parent frame at q = 0; the hinge axis is in the body frame.
 *   The base frame origin is the point the reference reports as
 *   `robot_body.pose().xyz()` (bullet_utils.py:104).
 *   All reals are fp32 so that every implementation starts from identical
 *   constants; the f64 oracle widens them.
 */
#ifndef MOCCA_MODEL_H
#define MOCCA_MODEL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MOCCA_MODEL_MAGIC 0x41434F4Du /* "MOCA" */
#define MOCCA_MODEL_VERSION 13u

#define MOCCA_MAX_BODIES 24
#define MOCCA_MAX_GEOMS 32
#define MOCCA_MAX_PAIRS 192
#define MOCCA_MAX_FEET 4
#define MOCCA_MAX_SLOTS 40   /* terrain contact slots (warm-start impulses) */
#define MOCCA_MAX_PLANKS 4   /* rendered_step_count: 3 (Walker3DStepperEnv, env_locomotion.py:345) / 4 (LaikagoStepperEnv, :904) */
#define MOCCA_MAX_TERRAIN_STEPS 20
#define MOCCA_MAX_CLOSURES 2
#define MOCCA_MAX_CTRL 16
#define MOCCA_TRAJ_STRIDE 32 /* floats per frame of the Cassie motion table (mocca_set_trajectory) */

enum { MOCCA_GEOM_SPHERE = 0, MOCCA_GEOM_CAPSULE = 1 };

/* MoccaModel.task_flags */
enum {
  MOCCA_TASKF_NEVER_DONE = 1,      /* Walker2DCustomEnv.step forces done = False (env_locomotion.py:302-309); TimeLimit still applies */
  MOCCA_TASKF_RESET_TAIL_ZERO = 2, /* Walker2DCustomEnv.reset returns [robot_state, 0, 0] (env_locomotion.py:299-300)            */
  MOCCA_TASKF_BODY_CONTACT = 4,    /* LaikagoCustomEnv.calc_base_reward: tall_bonus = 0, and -1 + done as soon as a non-foot link
                                      touches the ground (env_locomotion.py:877-890)                                              */
  MOCCA_TASKF_QUADRUPED_STEPPER = 8, /* LaikagoStepperEnv.calc_base_reward (env_locomotion.py:928-979): posture penalty from the hip /
                                      knee angles, progress x 2, posture x 0.2, tall_bonus 2, done = (t > 240 and next step <= 4),
                                      -1 + done when a non-foot link touches a plank                                              */
  MOCCA_TASKF_STALE_RESET_CONTACTS = 16, /* Walker3DStepperEnv.reset (env_locomotion.py:484-499) calls calc_feet_state() right after
                                      robot.reset(), BEFORE the terrain is redrawn and next_step_index is rewound: Bullet has not stepped
                                      since the last frame of the episode before, so getContactPoints still returns that frame's manifolds
                                      [UNVERIFIED-BULLET: contacts are refreshed by stepSimulation only].  The new episode therefore starts
                                      with feet_contact = the old episode's last contact flags (they enter the first step's observation,
                                      :525) and with target_reached_count = 1 if a foot was on the cover of what was then the target plank.
                                      Set on every Stepper blob (the reference's behaviour); clear it for a clean start.            */
};

/* MoccaModel.plank_shape */
enum { MOCCA_PLANK_BOX = 0 /* Plank, LargePlank (bullet_objects.py:92-103) */, MOCCA_PLANK_CYLINDER = 1 /* Pillar (:86-89), axis = plank z */ };

/* MoccaModel.cassie_mode: which class of env_cassie.py the Cassie task runs */
enum {
  MOCCA_CASSIE_PLAIN = 0,        /* CassieEnv (env_cassie.py:284-479)                                                  */
  MOCCA_CASSIE_PHASE_MOCCA = 1,  /* CassiePhaseMoccaEnv (:630-642): mocap targets, CassieMocapRewEnv reward, 42 floats */
  MOCCA_CASSIE_PHASE_MIRROR = 2, /* CassiePhaseMirrorEnv (:645-660): the same, observation mirrored when phase > 0.5  */
};

/* task ids accepted by mocca_create() */
enum {
  MOCCA_TASK_WALKER3D_CUSTOM = 0,  /* env_locomotion.py:37-282; also Child3D (:317-327), Walker2D / Crab2D (:285-314), Laikago (:854-890) by blob */
  MOCCA_TASK_WALKER3D_STEPPER = 1, /* env_locomotion.py:330-840; also MikeStepperEnv (:843-851) with a Mike blob       */
  MOCCA_TASK_CASSIE = 2,           /* env_cassie.py:284-479 (CassieEnv, 3-D) */
  MOCCA_TASK_WALKER3D_PLANNER = 3, /* env_locomotion.py:982-1128 (Walker3DPlannerEnv; MikePlannerEnv :1131-1133 with a Mike blob): the robot
                                      walks on a height field (bullet_objects.py:338-441, attached with mocca_set_heightfield) towards a
                                      target drawn once per episode; the low-level policy that turns the planner's 15 numbers into the 21
                                      joint actions is external (a pickled network, :1022-1033): the kernel takes the 21 actions */
};

typedef struct MoccaModel {
  uint32_t magic;
  uint32_t version;
  int32_t n_bodies; /* 1 + n_joints */
  int32_t n_joints;
  int32_t n_geoms;
  int32_t n_pairs; /* self-collision candidate pairs */
  int32_t n_feet;
  int32_t n_slots; /* terrain contact slots = spheres + 2*capsules */

  /* ---- topology ---- */
  int32_t parent[MOCCA_MAX_BODIES];    /* parent[0] = -1 */
  uint32_t anc_mask[MOCCA_MAX_BODIES]; /* bit b' set iff body b' (>=1) is b or an ancestor of b */
  int32_t depth[MOCCA_MAX_BODIES];     /* number of joints between base and b */

  /* ---- joints (index = body, entry 0 unused) ---- */
  float jpos[MOCCA_MAX_BODIES][3];
  float jrot[MOCCA_MAX_BODIES][9]; /* row-major, parent <- body at q=0; entry 0 = identity (the kinematics walk multiplies by it past the end of a path) */
  float jaxis[MOCCA_MAX_BODIES][3];
  float jlo[MOCCA_MAX_BODIES];
  float jhi[MOCCA_MAX_BODIES];
  float jdamp[MOCCA_MAX_BODIES];
  float jarm[MOCCA_MAX_BODIES];
  float gain[MOCCA_MAX_BODIES]; /* torque per unit action, robots.py:168 */

  /* ---- inertial (index = body) ---- */
  float mass[MOCCA_MAX_BODIES];
  float com[MOCCA_MAX_BODIES][3];
  float inertia[MOCCA_MAX_BODIES][6]; /* xx yy zz xy xz yz about com, body axes */

  /* ---- collision geoms ---- */
  int32_t g_body[MOCCA_MAX_GEOMS];
  int32_t g_type[MOCCA_MAX_GEOMS];
  int32_t g_slot[MOCCA_MAX_GEOMS];    /* first terrain slot of this geom */
  int32_t g_terrain[MOCCA_MAX_GEOMS]; /* 1 if the filter lets it touch static terrain */
  int32_t g_foot[MOCCA_MAX_GEOMS];    /* index into foot_body if the geom belongs to that foot's LINK (robots.py:74-86), else -1 */
  float g_radius[MOCCA_MAX_GEOMS];
  float g_p1[MOCCA_MAX_GEOMS][3]; /* body frame; sphere centre / capsule end 1 */
  float g_p2[MOCCA_MAX_GEOMS][3]; /* capsule end 2 (= p1 for spheres) */
  float g_friction[MOCCA_MAX_GEOMS];

  int32_t pair_a[MOCCA_MAX_PAIRS];
  int32_t pair_b[MOCCA_MAX_PAIRS];

  int32_t foot_body[MOCCA_MAX_FEET]; /* robots.py:232 foot_names order: right, left */
  float foot_point[MOCCA_MAX_FEET][3]; /* the foot LINK's centre of mass in the frame of foot_body (getLinkState()[0],
                                          bullet_utils.py:106): the body's own COM, except where the foot link is a fixed child
                                          merged into its parent (Laikago's toes) */

  /* ---- physics parameters (bullet_utils.py:340-350, env_base.py:78-83) ---- */
  float gravity;        /* 9.8 */
  float dt;             /* substep, 1/240 */
  int32_t n_substeps;   /* 4 */
  int32_t n_iters;      /* 5 */
  float erp;            /* 0.9  setDefaultContactERP */
  float contact_margin; /* contacts exist below this gap */
  float lin_damp;       /* link damping, btMultiBody m_linearDamping: every body (base and links) is dragged by m v (k + k |v|) through its COM */
  float ang_damp;       /* ... and by the torque Ic w (k + k |w|), m_angularDamping (v13; up to v12: base only, k only)                       */
  float max_qd;         /* joint velocity clamp */
  float warmstart;      /* fraction of last substep's normal impulse a terrain contact starts from; 0 disables (the compiled models: 0, see model.py) */
  float ground_friction;/* 0.8  bullet_utils.py:371 */
  float plank_friction; /* 1.0  bullet_objects.py:68 */
  float plank_stiffness;/* 30000 */
  float plank_damping;  /* 1000 */
  float plank_half[3];  /* half extents of the scaled LargePlank slab */
  float limit_slack;    /* joint-limit rows are built when predicted gap < slack */
  float plank_com_z;    /* z of the plank base link's inertial frame in the plank frame (bullet_objects.py:62) */

  /* ---- task constants ---- */
  float init_q[MOCCA_MAX_BODIES]; /* robots.py:296-302 "running_start", index = body */
  float init_pos[3];              /* robots.py:276 / env_locomotion.py:339 */
  float control_dt;               /* 1/60, scene.dt (bullet_utils.py:296) */
  float termination_height;       /* 0.7   env_locomotion.py:44 */
  float electricity_cost;         /* 4.5   env_locomotion.py:54 */
  float stall_torque_cost;        /* 0.225 */
  float joints_at_limit_cost;     /* 0.1   */
  int32_t max_episode_steps;      /* 1000  __init__.py:55 */
  int32_t mirror_right[9];        /* robots.py:282-284 (joint indices, 0-based) */
  int32_t mirror_left[9];         /* robots.py:285-287 */
  int32_t mirror_neg[2];          /* robots.py:288 */
  int32_t n_mirror_side;
  int32_t n_mirror_neg;
  int32_t max_contacts;           /* contacts kept per substep (priority: terrain slots, then self pairs) */
  int32_t max_rows;               /* constraint rows per substep: limits, closures, then 3 per contact */

  /* ---- point-to-point loop closures, env_cassie.py:114-137 (createConstraint JOINT_POINT2POINT) ---- */
  int32_t n_closures;
  int32_t cl_body_a[MOCCA_MAX_CLOSURES];
  int32_t cl_body_b[MOCCA_MAX_CLOSURES];
  float cl_point_a[MOCCA_MAX_CLOSURES][3]; /* pivot in body a's frame */
  float cl_point_b[MOCCA_MAX_CLOSURES][3];

  /* ---- Cassie low-level PD controller, env_cassie.py:287-319,380-393,433-459 ---- */
  int32_t n_ctrl;                     /* 12 = 10 powered joints + 2 knee_to_shin springs */
  int32_t n_llc;                      /* llc_frame_skip: PD + physics iterations per env.step (50) */
  int32_t ctrl_body[MOCCA_MAX_CTRL];  /* body of controlled joint k (powered joints first, then springs) */
  float ctrl_kp[MOCCA_MAX_CTRL];
  float ctrl_kd[MOCCA_MAX_CTRL];
  float ctrl_base[MOCCA_MAX_CTRL];    /* residual-control offset: base angle for powered joints, 0 for springs */
  float torque_limit[MOCCA_MAX_BODIES]; /* |torque| cap per body's joint (power_coef), env_cassie.py:41-56,225-230 */
  int32_t n_ordered;                  /* the reference's `ordered_joints` (14), env_cassie.py:160-199 */
  int32_t ordered_body[MOCCA_MAX_CTRL];
  int32_t ctrl_oidx[MOCCA_MAX_CTRL];  /* index of controlled joint k within ordered_body (env_cassie.py:59-60) */
  float jvel_alpha;                   /* 0.2, env_cassie.py:319 */
  float alive_height;                 /* 0.6, env_cassie.py:406-412 */
  float cassie_target[3];             /* (1000, 0, 0), env_cassie.py:366 */
  float init_quat[4];                  /* base orientation at reset, xyzw (robots.py:199-200; "crawl" pose :316-318) */
  int32_t task_flags;                 /* MOCCA_TASKF_*: quirks of the planar Custom envs (env_locomotion.py:285-314) */

  /* ---- Stepper terrain and task parameters: class attributes of Walker3DStepperEnv (env_locomotion.py:338-351,367-385)
   *      and their LaikagoStepperEnv overrides (:894-926); lookahead is 2 in both ---- */
  int32_t n_planks;             /* rendered_step_count            3    / 4    */
  int32_t lookbehind;           /*                                1    / 2    (also the first next_step_index, :499) */
  int32_t plank_shape;          /* MOCCA_PLANK_*: plank_half = half extents (box) or (radius, radius, half height) (cylinder) */
  float step_radius;            /*                                0.25 / 0.16 */
  float init_step_separation;   /*                                0.75 / 0.45 */
  float dist_range[2];          /*                           0.65 1.25 / 0.45 0.75 */
  float pitch_range_deg;        /* +-                             30   / 20   */
  float yaw_range_deg;          /* +-                             20   / 20   */
  float tilt_range_deg;         /* +-                             15   / 10   */
  float step_bonus_smoothness;  /*                                1    / 6    (:686) */
  float term_height_cur[2];     /* terminal_height_curriculum = linspace(a, b, 10):   0.75 0.45 / 0.20 0.0 */
  float gain_cur[2];            /* applied_gain_curriculum    = linspace(a, b, 10):   1.0  1.2  / 1.0  1.0 */
  float init_vel[3];            /* robot_init_velocity            None / (0.5, 0, 0.25)  (:340,901) */
  int32_t planar;               /* CassieEnv(planar=True) (env_cassie.py:326-341): base held in the x-z plane by three bilateral
                                   rows (v_y, omega_x, omega_z) -- stands in for the missing cassie_collide_2d.urdf (:279-282) */

  /* ---- Cassie mocap / phase envs (env_cassie.py:481-660); the motion itself is attached with mocca_set_trajectory ---- */
  int32_t cassie_mode;        /* MOCCA_CASSIE_*                                                                          */
  int32_t cassie_rsi;         /* rsi: reset at a random frame of the motion (env_cassie.py:331,364,585-588)              */
  int32_t residual_control;   /* the action is added to the motion's angles (1) or to zero (0), env_cassie.py:434-443    */
  int32_t rod_body[4];        /* bodies of fixed_{right,left}_achilles_rod_joint_{z,y}, the order of resetJoints (:591-596) */
  float mocap_w[6];           /* weights of SpeedRew, JPosRew, JVelRew, OrientationRew, AngularSpeedRew, CoMRew (:484-493) */
  float mocap_speed;          /* 0.8, the forward speed SpeedRew asks for (:498)                                         */

  /* ---- Walker3DPlannerEnv / MikePlannerEnv (env_locomotion.py:982-1133) ---- */
  int32_t g_torso[MOCCA_MAX_GEOMS]; /* 1 if the geom belongs to the LINK robot_torso_name ("waist", :992) names: the episode ends when that
                                       link touches anything, terrain or robot (getContactPoints(linkIndexA=robot_torso_id), :1104-1110) */
  float target_range;               /* 16: walk target xy ~ U(-16, 16)^2, z = the height field under it (:1060-1062)                  */
  float fall_z;                     /* -5: "free falling off terrain" (:1108)                                                          */
  /* ---- contact manifolds ---- */
  int32_t manifold_max;             /* 0: every terrain slot within the margin is a contact.  k > 0: per LINK at most k terrain contacts
                                       survive -- Bullet keeps a 4-point manifold per pair of collision objects (btPersistentManifold,
                                       MANIFOLD_CACHE_SIZE 4) [UNVERIFIED-BULLET], so Cassie's twelve hull points per toe (one convex
                                       mesh in cassie_collide.urdf) give 4 contacts, not 12: the deepest, the one farthest from it,
                                       and the two farthest to either side of the line through those two                              */
  float erp_noncontact;             /* v13: error reduction of the rows that are not contacts -- joint limits, Cassie's point-to-point closures,
                                       the planar-base rows.  Bullet: infoGlobal.m_erp (0.2; pybullet's setDefaultContactERP only sets m_erp2,
                                       which the contact rows use): btMultiBodyConstraint::fillMultiBodyConstraint ("split impulse is not
                                       implemented yet for btMultiBody*": erp = m_erp) and btMultiBodyJointLimitConstraint  [UNVERIFIED-BULLET] */
  int32_t friction_cone;            /* v13: 1 = the two friction rows of a contact are solved together and clipped to the CIRCLE of radius
                                       mu * lambda_n (Bullet >= 2.87 "implicit cone friction", btMultiBodyConstraintSolver::
                                       resolveConeFrictionConstraintRows; pybullet's enableConeFriction, "cone is default");
                                       0 = one after the other, each clipped to +-mu * lambda_n (pyramid)          [UNVERIFIED-BULLET] */
  int32_t limit_at_violation;       /* v13: 1 = a joint-limit row exists only while the joint is AT or PAST its limit (btMultiBodyJointLimitConstraint::
                                       createConstraintRows: "if (penetration > 0) continue"), pushed back with erp_noncontact; 0 = a row exists from a
                                       predicted gap of limit_slack on and stops the joint at the limit within the step (the file's older form,
                                       whose positive-gap branch is still in the source)                                   [UNVERIFIED-BULLET] */
  float linear_slop;                /* Bullet's infoGlobal.m_linearSlop: added to every contact distance before the row is built (penetration = distance +
                                       slop, btMultiBodyConstraintSolver::setupMultiBodyContactConstraint) -- a contact shallower than the slop gets a gap
                                       row, a deeper one is corrected by erp x (depth - slop).  pybullet: setPhysicsEngineParameter(contactSlop=...),
                                       1e-5 m where the server sets its default [UNVERIFIED-BULLET].  0 in the compiled blobs (the term was not
                                       modelled before round 5 and moves nothing measurable: 1e-5 m x erp / dt = 2 mm/s of bias); a dump's
                                       engine_contactSlop sets it.  (Takes the first of the former four reserved words: blobs of version 13 read as 0.) */
  int32_t sweep_alternate;          /* 1: the rows that are not contacts (joint limits, closures, planar-base rows) are swept last-to-first in the even
                                       Gauss-Seidel iterations and first-to-last in the odd ones (btMultiBodyConstraintSolver::solveSingleIteration:
                                       `index = iteration & 1 ? j : size - 1 - j` over m_multiBodyNonContactConstraints); contact and friction rows
                                       always forward.  0: always forward (every blob before round 5, and the compiled ones).  A blob with the flag runs the
                                       64-row accuracy instance of the step kernel, the only one that carries the second visit sequence  [UNVERIFIED-BULLET] */
  int32_t reserved_[2];

  /* ---- derived lookup tables (model.py finalize_tables): one 16-byte load instead of chains of dependent loads ---- */
  float slot_tab[MOCCA_MAX_SLOTS][4];       /* radius, friction, bits(body | geom<<8 | end<<16 | margin_code<<17 (8 bits, x 2^-13 m) | terrain<<25 | (foot + 1)<<26 | torso<<29), bits(anc_mask[body]) */
  float gp_tab[2 * MOCCA_MAX_GEOMS][4];     /* geom end point in its body frame (x, y, z), bits(body) */
  float pair_tab[MOCCA_MAX_PAIRS][4];       /* bits(geom_a | geom_b<<5 | body_a<<10 | body_b<<15 | margin_code<<20), radius_a, radius_b,
                                               broad-phase reach = half_len_a + half_len_b + radius_a + radius_b (padded; + the pair's margin at run time) */
  float slot_margin[MOCCA_MAX_SLOTS];       /* g_margin of the slot's geom (or contact_margin), quantised to 2^-13 m like the code in slot_tab */
  float pair_margin[MOCCA_MAX_PAIRS];       /* min of the two geoms' margins */
  /* (the new arrays sit at the END of the record: the kernels' loads of the older fields keep their immediate offsets) */
  float g_margin[MOCCA_MAX_GEOMS];  /* v13: contact breaking threshold of the geom's Bullet link.  btCollisionDispatcher::getNewManifold uses the RELATIVE
                                       threshold (CD_USE_RELATIVE_CONTACT_BREAKING_THRESHOLD, on by default): min over the two collision objects of
                                       shape->getContactBreakingThreshold(gContactBreakingThreshold) = contact_margin x getAngularMotionDisc(), the disc
                                       being the half diagonal of the link shape's AABB + the distance of its centre from the link's inertial frame --
                                       3 to 6 mm for a walker's links, not 20 mm.  The ground plane, planks and the height field have larger discs: the
                                       robot link's value decides; a self pair takes the smaller of its two links'.  <= 0: contact_margin itself (absolute).
                                       [UNVERIFIED-BULLET] */
} MoccaModel;

/* ------------------------------------------------------------------------
 * Per-env dynamic state record (floats), used by get_state/set_state:
 *   [0:3] base position  [3:7] base quaternion (x,y,z,w)
 *   [7:10] base linear velocity (world)  [10:13] base angular velocity (world)
 *   [13:13+nj] q   [13+nj:13+2nj] qd   then n_slots warm-start normal impulses
 * ------------------------------------------------------------------------ */
#define MOCCA_STATE_BASE 13
#define MOCCA_STATE_DIM(nj, nslots) (13 + 2 * (nj) + (nslots))

/* Per-env task record: MOCCA_TASK_WORDS 32-bit words per env, get/set_task().  The comment of each word gives its class (f = float,
 * i = int32), then its length in words when it spans more than one, then the tasks that use it.  Entries at the same index are aliases:
 * the env's task decides what the word holds.  (tests/test_task_record.py holds mocca_envs_amd/model.py TASK_RECORD to this enum.) */
enum MoccaTaskWord {
  MOCCA_TW_WALK_TARGET_X = 0,         /* f     walkers: walk_target */
  MOCCA_TW_WALK_TARGET_Y = 1,         /* f     walkers */
  MOCCA_TW_WALK_TARGET_Z = 2,         /* f     walkers */
  MOCCA_TW_LINEAR_POTENTIAL = 3,      /* f     all (Cassie: its potential, env_cassie.py:348-354) */
  MOCCA_TW_ANGULAR_POTENTIAL = 4,     /* f     walkers */
  MOCCA_TW_CLOSE_COUNT = 5,           /* i     Custom */
  MOCCA_TW_STOP_FRAMES = 6,           /* f     Custom */
  MOCCA_TW_DONE = 7,                  /* i     all: sticky */
  MOCCA_TW_T = 8,                     /* i     all: steps this episode */
  MOCCA_TW_EPISODE = 9,               /* i     all */
  MOCCA_TW_DRAW = 10,                 /* i     all: draw counter of the episode's random stream */
  MOCCA_TW_MIRRORED = 11,             /* i     walkers */
  MOCCA_TW_FEET_CONTACT_0 = 12,       /* f     walkers */
  MOCCA_TW_FEET_CONTACT_1 = 13,       /* f     walkers */
  MOCCA_TW_DIST = 14,                 /* f     Custom */
  MOCCA_TW_ANGLE = 15,                /* f     Custom */
  MOCCA_TW_NEXT_STEP_INDEX = 16,      /* i     Stepper */
  MOCCA_TW_TARGET_REACHED_COUNT = 17, /* i     Stepper */
  MOCCA_TW_STOP_ON_NEXT_STEP = 18,    /* i     Stepper */
  MOCCA_TW_SET_STOP_ON_NEXT_STEP = 19, /* i     Stepper */
  MOCCA_TW_CURRICULUM = 20,           /* i     Stepper */
  MOCCA_TW_APPLIED_GAIN = 21,         /* f     all */
  MOCCA_TW_PREV_BODY_X = 22,          /* f     walkers */
  MOCCA_TW_LAST_ROWS = 23,            /* i     all: constraint rows of the last physics substep (issue-priority hint for the next step: timing only) */
  MOCCA_TW_FEET_CONTACT_2 = 24,       /* f     quadrupeds (n_feet == 4) */
  MOCCA_TW_JVEL = 24,                 /* f 14  Cassie: filtered joint speeds jvel[14] (env_cassie.py:451-468) */
  MOCCA_TW_FEET_CONTACT_3 = 25,       /* f     quadrupeds */
  MOCCA_TW_COVER = 26,                /* f     Stepper: cover mask of the last substep's contacts, as a float (MOCCA_TASKF_STALE_RESET_CONTACTS) */
  MOCCA_TW_REWARD_WEIGHTS = 30,       /* f 8   Stepper: reward weights of this step (MOCCA_PARAM_RANDOM_REWARD, env_locomotion.py:533-547) */
  MOCCA_TW_INITIAL_Z = 38,            /* f     Cassie */
  MOCCA_TW_ISTEP = 39                 /* i     Cassie: mocap_time = istep * control_step / llc_frame_skip (env_cassie.py:359-360) */
};
#define MOCCA_TASK_WORDS 40

#ifdef __cplusplus
}
#endif
#endif /* MOCCA_MODEL_H */
