/*
 * zbot_base_inertia.h — the manager task's startup events events.add_base_mass
 * (randomize_rigid_body_mass) and events.base_com (randomize_rigid_body_com) of the reference's base
 * cfg (zbotlab_env_cfg.py): a mass and a centre of mass of the base link per env. Included by zbot.h;
 * do not include it on its own.
 *
 * Kept out of zbot.h itself for the reason zbot_manager_events.h is: zb_model, zb_task_cfg and the
 * state rows are the surface the CPU oracle mirrors, and they do not change. The per-env mass
 * properties live in a library-owned side buffer that zb_create allocates for manager handles. A handle
 * that never calls zb_set_base_inertia launches the same step kernels and computes the same bits as
 * before.
 *
 * Semantics (Isaac Lab's, per env): the base link's mass m' is given; with recompute_inertia its own
 * inertia tensor about its COM is multiplied by m' / (authored mass), otherwise kept. The COM offset
 * (link frame) is added to the authored COM; the link's tensor about its COM is unchanged by it (PhysX
 * keeps the inertia about the COM). The composite rigid body that holds the base link (the links
 * joined to it by fixed joints) is then summed again by the parallel-axis rule, in fp64, rounded to
 * fp32 once: mass, COM and inertia about the COM in the body frame, the layout of zb_model's
 * body_mass / body_com / body_inertia rows of that body, plus the base link's COM in the body frame
 * (zb_model.link_com of the base link).
 *
 * What reads the per-env values while the feature is on: the articulated-body pass of every substep of
 * zb_step (the build zb_m_dr_step_kernel of the manager step kernel, events compiled in; a handle
 * with the events off runs it with all-off event parameters) and of zb_physics_substeps; the base
 * link's COM velocity behind the command metrics; the interval push, which acts at the per-env COM.
 * What does not: the critic observation's contact-force scale stays 1 / (the nominal robot's weight)
 * (zbot_critic_obs.h), and the per-env mass / COM are not part of any observation group.
 */
#ifndef ZBOT_BASE_INERTIA_H_
#define ZBOT_BASE_INERTIA_H_

/* The authored base link and the rest of its composite body, which zb_model (composites only) does
 * not carry; fp64, body frame. */
typedef struct zb_base_link {
  double mass;             /* the base link's authored mass */
  double com[3];           /* its COM, body frame (= zb_model.link_com of the base link) */
  double rot[9];           /* link frame -> body frame rotation, row major (zb_model.link_rot) */
  double inertia[6];       /* its tensor about its COM, body axes: xx yy zz xy xz yz */
  double rest_mass;        /* the body's other links as one part: mass (0: none), */
  double rest_com[3];      /* COM (body frame) */
  double rest_inertia[6];  /* and tensor about that COM */
} zb_base_link;

#define ZB_BI_ROWS 12 /* {com xyz, mass}, {Ixx Iyy Izz Ixy}, {Ixz Iyz 0 0} */

/* Manager task only (another task: -1 and zb_last_error, before any launch). Host only; needs
 * mass > 0. Call once before the first zb_set_base_inertia. */
int zb_set_base_link(zb_handle h, const zb_base_link* link);

/* mass_com: device float[N][4], the base link's mass and its COM offset xyz (link frame) per env; NULL
 * switches the feature off again (the next zb_step launches what it launched before). Manager task
 * only, after zb_set_base_link (otherwise -1 and zb_last_error, before any launch). One small launch on
 * `stream` composes the rows into the side buffer; no allocation, no synchronisation, no host read of
 * device data: graph-safe like zb_set_manager_events. A mass that is not positive and finite (or a
 * non-finite offset) cannot be refused here without reading device memory: the kernel keeps that
 * env's previous rows and raises a device flag, which the next zb_base_inertia_check reports. */
int zb_set_base_inertia(zb_handle h, const float* mass_com, int recompute_inertia, void* stream);

/* 1 while the handle's next zb_step launches zb_m_dr_step_kernel (zb_kernel_variant names the template
 * arguments it shares with the other two builds), else 0. Host only. */
int zb_base_inertia_active(zb_handle h);

/* The host-side query of the device flag: synchronises `stream`, returns 0 when every mass given to
 * zb_set_base_inertia so far was accepted, else -1 with zb_last_error (and clears the flag). */
int zb_base_inertia_check(zb_handle h, void* stream);

/* The composed rows as device float[ZB_BI_ROWS][N] (tests): rows 0..3 {com xyz, mass}, 4..7
 * {Ixx Iyy Izz Ixy}, 8..11 {Ixz Iyz 0 0}. The nominal body's rows until the first set. */
int zb_get_base_inertia(zb_handle h, float* dst, void* stream);

/* The per-env base-link COM in the body frame as device float[3][N] (tests). */
int zb_get_base_link_com(zb_handle h, float* dst, void* stream);

#endif /* ZBOT_BASE_INERTIA_H_ */
