/*
 * mjw_amd.h -- C ABI of the MI355X batched MuJoCo stepper (libmjw_amd.so).
 *
 * Drop-in boundary for the `mjw.step(m, d)` path of mujoco_warp.  Each entry
 * point replaces one reference function (file:line in mujoco_warp/_src):
 *
 *   mjw_step              <- forward.step                 forward.py:1003-1018
 *   mjw_forward           <- forward.forward              forward.py:972-1000
 *   mjw_fwd_position      <- forward.fwd_position         forward.py:513-537
 *   mjw_contact_rows      <- constraint.make_constraint   constraint.py:2718-2779 (contact rows again from
 *                            d.contact after a contactfilter callback, collision_driver.py:788-789)
 *   mjw_fwd_velocity      <- forward.fwd_velocity         forward.py:592-613
 *   mjw_fwd_actuation     <- forward.fwd_actuation        forward.py:836-927
 *   mjw_fwd_acceleration  <- forward.fwd_acceleration     forward.py:949-969
 *   mjw_solve             <- solver.solve                 solver.py:3296-3343
 *   mjw_euler             <- forward.euler                forward.py:326-354
 *   mjw_stage             <- smooth.kinematics / com_pos / camlight / tendon / crb / transmission /
 *                            com_vel / rne, passive.passive, constraint.make_constraint (one stage, below)
 *   mjw_sensor            <- sensor.sensor_pos/_vel/_acc  sensor.py:761,1377,2447
 *   mjw_ctrl_noise        <- benchmark.ctrl_noise         _src/benchmark.py:41-83
 *   mjw_rays              <- ray.rays (no render context) ray.py:1212-1312
 *   mjw_render            <- render.render (brute force over the geoms; textures: mjw_render_tex) render.py:515-830
 *   mjw_rays_bvh / mjw_render_bvh <- the same with a static BVH per mesh (no BVH over the geoms, none to refit)
 *   mjw_flex_refit / mjw_render_flex <- render.refit_bvh / render.render of a context made with render_flex
 *   mjw_render_tex        <- render.render of a context that has textures (use_textures; planes and meshes with texcoords)
 *   mjw_inverse           <- inverse.inverse's constraint + combine  inverse.py, solver.py init_context(grad=False)
 *   mjw_island            <- island.island (connected components by union-find, no tree x tree matrix) island.py:246-265
 *   mjw_fd_perturb / mjw_fd_difference <- no reference counterpart: MuJoCo's mjd_transitionFD around mjw_step (derivative_fd.py)
 *
 * Ownership: the caller owns every buffer (device pointers below); the library
 * never allocates or frees device memory and keeps no global mutable state.
 * All launches are asynchronous on the caller's HIP stream (graph capturable).
 * Return value: 0 on success, nonzero HIP error code otherwise
 * (mjw_last_error() gives the message).
 *
 * Field lists are X-macros: the Python host (mujoco_warp_amd/_lib.py) parses
 * them to build byte-identical ctypes structs.
 */
#ifndef MJW_AMD_H
#define MJW_AMD_H

#include <stdint.h>

#define MJW_ABI_VERSION 36

/* ---- model: int scalars ---- */
#define MJW_MODEL_INT_SCALARS(X)                                                                   \
  X(nq) X(nv) X(nu) X(na) X(nbody) X(njnt) X(ngeom) X(nsite) X(ncam) X(nlight) X(nmocap)          \
  X(nxn) X(nlevel) X(nlimited) X(nlimited_ball) X(nmaxcondim) X(nmaxpyramid) X(nv_pad) X(nJmom)    \
  X(neq) X(neq_cw)                                                                                 \
  X(nsensor) X(nsensordata) X(sensor_rne_postconstraint) X(nsensor_acc)                           \
  X(nxn_ccd) X(nxn_box) X(opt_ccd_iterations) X(ccd_epa_iterations)                                           \
  X(opt_integrator) X(opt_cone) X(opt_solver) X(opt_iterations) X(opt_ls_iterations)             \
  X(opt_disableflags) X(opt_enableflags) X(opt_broadphase_filter) X(opt_ls_parallel)               \
  X(is_sparse) X(nM) X(ntree) X(njrow)                                                             \
  X(nflex) X(nflexvert) X(nflexedge) X(nflexelem) X(nflexelemdata) X(nflexinc) X(nflexcg) X(nplane) \
  X(nflexelemedge) X(nflexshelldata)                                                               \
  X(nmesh) X(nmeshvert) X(ntendon) X(nwrap) X(nJten) X(ten_maxnnz) X(nmuscle) X(sp_nH)   \
  X(npair) X(ngravcomp) X(has_fluid) X(nten_spatial) X(act_maxnnz) X(nbodytrn) X(nsitetrn)             \
  X(nsensorcollision) X(nsensorccd) X(nhfield) X(nhfielddata) X(opt_contact_sensor_maxmatch)           \
  X(nmeshpoly) X(nmeshpolyvert) X(nmeshpolymap) X(nmaxpolygon) X(nmaxmeshdeg) X(nsensortaxel) X(nmeshnormal) X(nsensorcontact)

/* ---- model: float arrays, batchable (leading dim nb = 1 or nworld, indexed worldid % nb) ---- */
#define MJW_MODEL_REAL_ARRAYS(X)                                                                   \
  X(opt_timestep, 1) X(opt_tolerance, 1) X(opt_ls_tolerance, 1) X(opt_impratio_invsqrt, 1)        \
  X(opt_ccd_tolerance, 1)                                                                          \
  X(opt_gravity, 3) X(opt_magnetic, 3) X(stat_meaninertia, 1)                                      \
  X(opt_wind, 3) X(opt_density, 1) X(opt_viscosity, 1) X(opt_ls_parallel_min_step, 1)             \
  X(qpos0, nq) X(qpos_spring, nq)                                                                  \
  X(body_pos, nbody * 3) X(body_quat, nbody * 4) X(body_ipos, nbody * 3) X(body_iquat, nbody * 4) \
  X(body_mass, nbody) X(body_subtreemass, nbody) X(body_inertia, nbody * 3)                       \
  X(body_invweight0, nbody * 2) X(body_gravcomp, nbody)                                            \
  X(jnt_solref, njnt * 2) X(jnt_solimp, njnt * 5) X(jnt_pos, njnt * 3) X(jnt_axis, njnt * 3)      \
  X(jnt_stiffness, njnt) X(jnt_range, njnt * 2) X(jnt_actfrcrange, njnt * 2) X(jnt_margin, njnt)  \
  X(dof_solref, nv * 2) X(dof_solimp, nv * 5) X(dof_frictionloss, nv) X(dof_armature, nv)         \
  X(dof_damping, nv) X(dof_invweight0, nv)                                                         \
  X(geom_solmix, ngeom) X(geom_solref, ngeom * 2) X(geom_solimp, ngeom * 5) X(geom_size, ngeom * 3) \
  X(geom_aabb, ngeom * 6) X(geom_rbound, ngeom) X(geom_pos, ngeom * 3) X(geom_quat, ngeom * 4)    \
  X(geom_friction, ngeom * 3) X(geom_margin, ngeom) X(geom_gap, ngeom) X(geom_fluid, ngeom * 12)  \
  X(site_pos, nsite * 3) X(site_quat, nsite * 4) X(site_size, nsite * 3)                                                \
  X(cam_pos, ncam * 3) X(cam_quat, ncam * 4) X(cam_poscom0, ncam * 3) X(cam_pos0, ncam * 3)       \
  X(cam_mat0, ncam * 9) X(cam_fovy, ncam) X(cam_sensorsize, ncam * 2) X(cam_intrinsic, ncam * 4)    \
  X(light_pos, nlight * 3) X(light_dir, nlight * 3) X(light_poscom0, nlight * 3)                  \
  X(light_pos0, nlight * 3) X(light_dir0, nlight * 3)                                              \
  X(actuator_dynprm, nu * 10) X(actuator_gainprm, nu * 10) X(actuator_biasprm, nu * 10)           \
  X(actuator_ctrlrange, nu * 2) X(actuator_forcerange, nu * 2) X(actuator_actrange, nu * 2)       \
  X(actuator_gear, nu * 6) X(actuator_acc0, nu) X(actuator_lengthrange, nu * 2) X(actuator_cranklength, nu)                   \
  X(eq_solref, neq * 2) X(eq_solimp, neq * 5) X(eq_data, neq * 11)                               \
  X(sensor_cutoff, nsensor)                                                                        \
  X(flex_radius, nflex) X(flex_margin, nflex) X(flex_damping, nflex) X(flex_friction, nflex * 3)  \
  X(flexedge_length0, nflexedge) X(flexedge_invweight0, nflexedge)                                \
  X(flex_stiffness, nflexelem * 21) X(flex_bending, nflexedge * 17) X(mesh_normal, nmeshnormal * 3) \
  X(mesh_vert, nmeshvert * 3) X(hfield_size, nhfield * 4) X(hfield_data, nhfielddata)             \
  X(mesh_polynormal, nmeshpoly * 3)                                                                \
  X(tendon_stiffness, ntendon) X(tendon_damping, ntendon) X(tendon_frictionloss, ntendon)          \
  X(tendon_armature, ntendon) X(tendon_margin, ntendon) X(tendon_range, ntendon * 2)               \
  X(tendon_lengthspring, ntendon * 2) X(tendon_solref_lim, ntendon * 2) X(tendon_solimp_lim, ntendon * 5) \
  X(tendon_solref_fri, ntendon * 2) X(tendon_solimp_fri, ntendon * 5) X(tendon_invweight0, ntendon)  \
  X(tendon_actfrcrange, ntendon * 2) X(tendon_length0, ntendon) X(wrap_prm, nwrap) X(wrap_pulley_scale, nwrap)                                          \
  X(pair_solref, npair * 2) X(pair_solreffriction, npair * 2) X(pair_solimp, npair * 5)           \
  X(pair_margin, npair) X(pair_gap, npair) X(pair_friction, npair * 5)

/* ---- model: int arrays (never batched) ---- */
#define MJW_MODEL_INT_ARRAYS(X)                                                                    \
  X(body_parentid, nbody) X(body_rootid, nbody) X(body_weldid, nbody) X(body_mocapid, nbody)      \
  X(body_jntnum, nbody) X(body_jntadr, nbody) X(body_dofnum, nbody) X(body_dofadr, nbody)         \
  X(body_subtree_end, nbody) X(body_level, nbody) X(level_body, nbody) X(level_adr, nlevel + 1)    \
  X(jnt_type, njnt) X(jnt_qposadr, njnt) X(jnt_dofadr, njnt) X(jnt_bodyid, njnt)                  \
  X(jnt_limited, njnt) X(jnt_actfrclimited, njnt) X(jnt_limited_slide_hinge_adr, nlimited)        \
  X(jnt_limited_ball_adr, nlimited_ball) X(jnt_actgravcomp, njnt)                                 \
  X(body_geomadr, nbody) X(body_geomnum, nbody) X(body_fluid_ellipsoid, nbody)                    \
  X(dof_bodyid, nv) X(dof_jntid, nv) X(dof_parentid, nv)                                           \
  X(geom_type, ngeom) X(geom_condim, ngeom) X(geom_bodyid, ngeom) X(geom_priority, ngeom)         \
  X(site_bodyid, nsite) X(site_type, nsite)                                                                      \
  X(cam_mode, ncam) X(cam_bodyid, ncam) X(cam_targetbodyid, ncam) X(cam_resolution, ncam * 2)     \
  X(light_mode, nlight) X(light_bodyid, nlight) X(light_targetbodyid, nlight)                     \
  X(actuator_trntype, nu) X(actuator_dyntype, nu) X(actuator_gaintype, nu)                        \
  X(actuator_biastype, nu) X(actuator_trnid, nu * 2) X(actuator_actadr, nu) X(actuator_actnum, nu) \
  X(actuator_ctrllimited, nu) X(actuator_forcelimited, nu) X(actuator_actlimited, nu)             \
  X(actuator_actearly, nu)                                                                         \
  X(nxn_geom_pair, nxn * 2) X(nxn_pairid, nxn * 2) X(nxn_ccdid, nxn) X(pair_dim, npair)            \
  X(eq_type, neq) X(eq_obj1id, neq) X(eq_obj2id, neq) X(eq_objtype, neq)                                             \
  X(sensor_type, nsensor) X(sensor_datatype, nsensor) X(sensor_objtype, nsensor)                   \
  X(sensor_objid, nsensor) X(sensor_reftype, nsensor) X(sensor_refid, nsensor)                     \
  X(sensor_adr, nsensor) X(sensor_dim, nsensor) X(sensor_needstage, nsensor) X(sensor_intprm, nsensor * 3) \
  X(sensor_collision_adr, nsensor) X(sensor_collision_num, nsensor) X(sensor_collision_pair, nsensorcollision * 4) \
  X(M_rownnz, nv) X(M_rowadr, nv) X(M_colind, nM) X(tree_dofadr, ntree + 1)                        \
  X(flex_dim, nflex) X(flex_vertadr, nflex) X(flex_edgeadr, nflex) X(flex_edgenum, nflex)          \
  X(flex_elemadr, nflex) X(flex_elemnum, nflex) X(flex_elemdataadr, nflex) X(flex_elemedgeadr, nflex) \
  X(flex_condim, nflex) X(flex_cgeomadr, nflex + 1) X(flex_cgeom, nflexcg) X(plane_geom, nplane)   \
  X(flex_vertbodyid, nflexvert) X(flex_vertflexid, nflexvert) X(flex_edge, nflexedge * 2)          \
  X(flex_edgeflap, nflexedge * 2) X(flex_elem, nflexelemdata) X(flex_elemedge, nflexelemedge)      \
  X(flex_shellnum, nflex) X(flex_shelldataadr, nflex) X(flex_shell, nflexshelldata)               \
  X(taxel_vertadr, nsensortaxel) X(taxel_sensorid, nsensortaxel) X(mesh_normaladr, nmesh) X(mesh_normalnum, nmesh) \
  X(flexvert_incadr, nflexvert + 1) X(flexvert_inc, nflexinc)                                     \
  X(mesh_vertadr, nmesh) X(mesh_vertnum, nmesh) X(geom_dataid, ngeom)                            \
  X(mesh_polyadr, nmesh) X(mesh_polynum, nmesh) X(mesh_polyvertadr, nmeshpoly) X(mesh_polyvertnum, nmeshpoly) \
  X(mesh_polyvert, nmeshpolyvert) X(mesh_polymapadr, nmeshvert) X(mesh_polymapnum, nmeshvert) X(mesh_polymap, nmeshpolymap) \
  X(hfield_nrow, nhfield) X(hfield_ncol, nhfield) X(hfield_adr, nhfield)                          \
  X(tendon_adr, ntendon) X(tendon_num, ntendon) X(tendon_limited, ntendon) X(tendon_actfrclimited, ntendon) \
  X(wrap_objid, nwrap) X(wrap_type, nwrap) X(ten_J_rownnz, ntendon) X(ten_J_rowadr, ntendon) X(ten_J_colind, nJten)

/* ---- data: float arrays, (nworld, count) world-major like mujoco_warp types.Data ----
 * Sparse models (is_sparse, the reference's io.py:67-74 switch) store qM / qLD as (nworld, nM) rows of
 * ancestors ascending then the diagonal (M_rowadr / M_colind), and efc_J as (nworld, njmax_pad, njrow)
 * stored slot-major (slot k of row r at [k * njmax_pad + r]) with efc_J_colind / efc_J_rownnz; dense models keep qM (nv_pad, nv_pad), qLD (nv, nv), efc_J
 * (njmax_pad, nv_pad).  sp_* / efc_JT_* / sp_cnt are sparse-path workspace (size 0 when dense); ncon_world holds a
 * world's contact-pool range (first slot, count / span): the sparse path's, and the dense contact-rows pass's;
 * sp_idx16 holds the CG's 16-bit copies of efc_J_colind and of the transposed index's rows (two uint16 per int).
 * world_order / world_key: the dense path's longest-first world order (a permutation of the worlds, rebuilt
 * every step from the previous step's solver iterations) and each world's iteration bucket.
 * qfrc_inverse: the inverse dynamics force mjw_inverse writes (ABI 36). */
#define MJW_DATA_REAL_ARRAYS(X)                                                                    \
  X(time, 1) X(qpos, nq) X(qvel, nv) X(act, na) X(ctrl, nu) X(qacc_warmstart, nv)                 \
  X(qfrc_applied, nv) X(xfrc_applied, nbody * 6) X(mocap_pos, nmocap * 3) X(mocap_quat, nmocap * 4) \
  X(qacc, nv) X(act_dot, na) X(energy, 2)                                                          \
  X(xpos, nbody * 3) X(xquat, nbody * 4) X(xmat, nbody * 9) X(xipos, nbody * 3) X(ximat, nbody * 9) \
  X(xanchor, njnt * 3) X(xaxis, njnt * 3) X(geom_xpos, ngeom * 3) X(geom_xmat, ngeom * 9)         \
  X(site_xpos, nsite * 3) X(site_xmat, nsite * 9) X(cam_xpos, ncam * 3) X(cam_xmat, ncam * 9)     \
  X(light_xpos, nlight * 3) X(light_xdir, nlight * 3)                                              \
  X(subtree_com, nbody * 3) X(subtree_linvel, nbody * 3) X(subtree_angmom, nbody * 3) X(cdof, nv * 6) X(cinert, nbody * 10) X(crb, nbody * 10)              \
  X(qM, nv_pad * nv_pad) X(qLD, nv * nv)                                                           \
  X(actuator_length, nu) X(actuator_moment, nJmom) X(actuator_velocity, nu) X(actuator_force, nu) \
  X(cvel, nbody * 6) X(cdof_dot, nv * 6) X(qfrc_bias, nv) X(qfrc_spring, nv) X(qfrc_damper, nv)   \
  X(qfrc_gravcomp, nv) X(qfrc_fluid, nv) X(qfrc_passive, nv) X(qfrc_actuator, nv) X(qfrc_smooth, nv) \
  X(qacc_smooth, nv) X(qfrc_constraint, nv) X(cacc, nbody * 6) X(cfrc_int, nbody * 6)             \
  X(cfrc_ext, nbody * 6)                                                                           \
  X(efc_J, njmax_pad * nv_pad) X(efc_pos, njmax) X(efc_margin, njmax) X(efc_D, njmax_pad)         \
  X(efc_vel, njmax) X(efc_aref, njmax) X(efc_frictionloss, njmax) X(efc_force, njmax)             \
  X(efc_Ma, nv) X(sensordata, nsensordata) X(ccd_out, nxn_ccd * 32)                                 \
  X(qpos_t0, nq) X(qvel_t0, nv) X(act_t0, na) X(qvel_rk, nv) X(qacc_rk, nv) X(act_dot_rk, na)     \
  X(flexvert_xpos, nflexvert * 3) X(flexedge_length, nflexedge) X(flexedge_velocity, nflexedge)   \
  X(flexedge_J, nflexedge * 6) X(flex_frc, nflexelem * 12 + nflexedge * 12)                       \
  X(sp_body, nbody * 6) X(sp_vec, nv * 10) X(sp_row, njmax * 3) X(sp_LD, nM) X(sp_H, sp_nH * sp_nH) \
  X(efc_JT_val, njmax_pad * njrow)                                                                 \
  X(ten_length, ntendon) X(ten_velocity, ntendon) X(ten_J, nJten)                                 \
  X(qfrc_inverse, nv)

/* ---- data: int arrays, (nworld, count) ---- */
#define MJW_DATA_INT_ARRAYS(X)                                                                     \
  X(ne, 1) X(nf, 1) X(nl, 1) X(nefc, 1) X(solver_niter, 1)                                         \
  X(moment_rownnz, nu) X(moment_rowadr, nu) X(moment_colind, nJmom)                                \
  X(efc_type, njmax) X(efc_id, njmax) X(efc_state, njmax_pad) X(eq_active, neq)                   \
  X(efc_J_colind, njmax_pad * njrow) X(efc_J_rownnz, njmax) X(efc_JT_rowind, njmax_pad * njrow)   \
  X(efc_JT_adr, nv + 1) X(sp_cnt, nv + 1) X(ncon_world, 2)                                        \
  X(sp_idx16, njmax_pad * njrow)                                                                   \
  X(world_order, 1) X(world_key, 1)

/* ---- contact pool: float arrays, (naconmax, count) ---- */
#define MJW_CONTACT_REAL_ARRAYS(X)                                                                 \
  X(contact_dist, 1) X(contact_pos, 3) X(contact_frame, 9) X(contact_includemargin, 1)            \
  X(contact_friction, 5) X(contact_solref, 2) X(contact_solreffriction, 2) X(contact_solimp, 5)

/* ---- contact pool: int arrays, (naconmax, count) ---- */
#define MJW_CONTACT_INT_ARRAYS(X)                                                                  \
  X(contact_dim, 1) X(contact_geom, 2) X(contact_efc_address, nmaxpyramid) X(contact_worldid, 1)  \
  X(contact_type, 1) X(contact_geomcollisionid, 1) X(contact_flex, 2) X(contact_vert, 2)

typedef struct mjw_model_t {
#define MJW_DECL_I(name) int32_t name;
#define MJW_DECL_RA(name, n) const float* name; int32_t name##_nb; int32_t name##_cnt;
#define MJW_DECL_IA(name, n) const int32_t* name;
  MJW_MODEL_INT_SCALARS(MJW_DECL_I)
  MJW_MODEL_REAL_ARRAYS(MJW_DECL_RA)
  MJW_MODEL_INT_ARRAYS(MJW_DECL_IA)
} mjw_model_t;

/* world-order workspace (mjw_data_t.sched): non-null enables the longest-first order (its words are spare since
   round 6: the counter-reset kernel histograms world_key itself) */
#define MJW_SCHED_BUCKETS 32
#define MJW_SCHED_WORDS (2 * MJW_SCHED_BUCKETS + 2)

typedef struct mjw_data_t {
  int32_t nworld;     /* worlds held by these buffers */
  int32_t njmax;      /* max constraint rows per world */
  int32_t njmax_pad;  /* padded row count of efc_J / efc_D / efc_state */
  int32_t naconmax;   /* contact pool capacity (all worlds) */
  int32_t world_offset; /* global id of world 0 (multi-GPU sharding); affects ctrl noise only */
  int32_t pad_;
  int32_t* nacon;      /* (1,) contacts written this step (may exceed naconmax) */
  int32_t* ncollision; /* (1,) broadphase pairs this step; when ncollision == nacon + 1 (one 8-B aligned pair,
                          as put_data allocates them) the step adds both with one 64-bit atomic per world */
  int32_t* sched;      /* (MJW_SCHED_WORDS,) world-order workspace of the dense path: histogram of
                        * the previous step's solver-iteration buckets, bucket cursors, valid flag */
#define MJW_DECL_DRA(name, n) float* name;
#define MJW_DECL_DIA(name, n) int32_t* name;
  MJW_DATA_REAL_ARRAYS(MJW_DECL_DRA)
  MJW_DATA_INT_ARRAYS(MJW_DECL_DIA)
  MJW_CONTACT_REAL_ARRAYS(MJW_DECL_DRA)
  MJW_CONTACT_INT_ARRAYS(MJW_DECL_DIA)
} mjw_data_t;

/* Model fields that only ray casting reads (mjw_rays).  They are kept out of mjw_model_t, which is passed by
 * value to every step kernel.  geom_rgba / mat_rgba are batchable like the model's float arrays: leading
 * dim nb = 1 or nworld, world w reads row w % nb.  mesh_face holds vertex indices local to each mesh. */
typedef struct mjw_ray_model_t {
  int32_t ngeom;      /* must equal mjw_model_t.ngeom */
  int32_t nmat;       /* materials */
  int32_t nmeshface;  /* triangles of all meshes */
  int32_t geom_rgba_nb;
  int32_t mat_rgba_nb;
  int32_t pad_;
  const int32_t* geom_group;   /* (ngeom,) */
  const int32_t* geom_matid;   /* (ngeom,) material id or -1 */
  const float* geom_rgba;      /* (geom_rgba_nb, ngeom, 4) */
  const float* mat_rgba;       /* (mat_rgba_nb, nmat, 4); may be NULL when nmat == 0 */
  const int32_t* mesh_face;    /* (nmeshface, 3); may be NULL when nmeshface == 0 */
  const int32_t* mesh_faceadr; /* (nmesh,) */
  const int32_t* mesh_facenum; /* (nmesh,) */
} mjw_ray_model_t;

/* A render context (mjw_render): which cameras are rendered at what resolution into which outputs, the tile
 * table of the launch, the lights' switches and the output buffers.  Every pointer is a device pointer.  Like
 * mjw_ray_model_t it stays out of mjw_model_t. */
typedef struct mjw_render_t {
  uint32_t group_mask;   /* bit g set: geoms of group g are drawn (exact match, groups 0..31) */
  int32_t use_shadows;   /* shadow rays for lights with castshadow */
  int32_t nrender;       /* rendered cameras (rows of the camera table) */
  int32_t ntile;         /* rows of the tile table; 0: nothing to render */
  int32_t tile_threads;  /* 256: tiles of 16 x 16 pixels; 64: one tile per camera, every camera <= 64 pixels */
  int32_t pad_;
  const int32_t* cam_id_map; /* (nrender,) camera id in the model */
  const int32_t* cam_res;    /* (nrender, 2) width, height */
  const int32_t* rgb_adr;    /* (nrender,) first pixel of the camera in a row of rgb, -1: output off */
  const int32_t* depth_adr;  /* (nrender,) likewise for depth */
  const int32_t* seg_adr;    /* (nrender,) likewise for seg */
  const int32_t* tile;       /* (ntile, 4) row of the camera table, x0, y0, 0; cameras without an output have none */
  const int32_t* light_type;       /* (nlight,) 0 spot, 1 directional, 2 point */
  const int32_t* light_active;     /* (nlight,) */
  const int32_t* light_castshadow; /* (nlight,) */
  int32_t* rgb;      /* (nworld, rgb_ld) packed a << 24 | r << 16 | g << 8 | b */
  float* depth;      /* (nworld, depth_ld) planar depth, 0: background */
  int32_t* seg;      /* (nworld, seg_ld) geom id, -1: background */
  int64_t rgb_ld, depth_ld, seg_ld; /* row lengths; the kernel writes no pixel at or past them */
} mjw_render_t;

/* The static mesh BVHs of a render context (mjw_rays_bvh, mjw_render_bvh): one binary tree per mesh, in the mesh's
 * frame, built on the host from the unbatched mesh_vert.  Every pointer is a device pointer.
 * node: 8 words per node, the box minimum (3 floats), the box maximum (3 floats) and two int32: an inner node holds
 * the left child and (right child | split axis << 29), children counted from the mesh's first node and always
 * greater than their parent; a leaf (second int <= 0) holds its first entry of tri, counted from the mesh's first
 * entry, and minus its number of triangles (at most leaf_size).  tri: face ids local to the mesh, grouped by leaf.
 * adr: per mesh its first node, its number of nodes, its first entry of tri (= mesh_faceadr) and its depth. */
typedef struct mjw_bvh_t {
  int32_t nmesh;      /* must equal mjw_model_t.nmesh */
  int32_t nnode;      /* nodes of all meshes */
  int32_t ntri;       /* entries of tri; must equal mjw_ray_model_t.nmeshface */
  int32_t leaf_size;  /* triangles per leaf at the most; at most 4 */
  int32_t max_depth;  /* levels of the deepest tree; at most 32 */
  int32_t min_faces;  /* meshes with fewer faces are intersected by the loop over their faces (same results) */
  const float* node;   /* (nnode, 8) */
  const int32_t* tri;  /* (ntri,) */
  const int32_t* adr;  /* (nmesh, 4) */
} mjw_bvh_t;

#ifdef __cplusplus
extern "C" {
#endif

int mjw_abi_version(void);
const char* mjw_last_error(void);
/* sizeof checks for the Python binding */
int mjw_sizeof_model(void);
int mjw_sizeof_data(void);
/* per-world LDS bytes the fused step needs for this model and njmax */
int mjw_lds_bytes(const mjw_model_t* m, int njmax);

/* stream: a hipStream_t (NULL = default stream) */
int mjw_step(const mjw_model_t* m, const mjw_data_t* d, void* stream);
/* mjw_step with timing: hipEvent_t handles recorded on `stream` before the forward kernel,
 * between the forward and the dense factor/solve/euler kernel, and after it (bench.py uses
 * this to time the dominant kernel live; on the generic path only ev_begin/ev_end bracket it).
 * No reference counterpart (the reference times with wp.ScopedTimer/event_trace, benchmark.py). */
int mjw_step_events(const mjw_model_t* m, const mjw_data_t* d, void* stream, void* ev_begin, void* ev_mid, void* ev_end);

/* mjw_step with a launch trace: events[0] is recorded on `stream` before the step and events[i + 1]
 * right after the step's i-th kernel launch (i < nevents - 1), kernel_ids[i] names that kernel
 * (mjw_kernel_name); *nlaunch = launches traced.  The events must exist (hipEventCreate).  bench.py
 * times every kernel of the step with it on the stream they run on.  No reference counterpart (the
 * reference's event_trace, benchmark.py, times its Warp kernels the same way). */
int mjw_step_trace(const mjw_model_t* m, const mjw_data_t* d, void* stream, void** events, int nevents, int* kernel_ids,
                   int* nlaunch);
const char* mjw_kernel_name(int kernel_id);

int mjw_forward(const mjw_model_t* m, const mjw_data_t* d, void* stream);
int mjw_fwd_position(const mjw_model_t* m, const mjw_data_t* d, void* stream);
int mjw_contact_rows(const mjw_model_t* m, const mjw_data_t* d, void* stream);
int mjw_fwd_velocity(const mjw_model_t* m, const mjw_data_t* d, void* stream);
int mjw_fwd_actuation(const mjw_model_t* m, const mjw_data_t* d, void* stream);
int mjw_fwd_acceleration(const mjw_model_t* m, const mjw_data_t* d, void* stream);
int mjw_solve(const mjw_model_t* m, const mjw_data_t* d, void* stream);
int mjw_euler(const mjw_model_t* m, const mjw_data_t* d, void* stream);
/* One stage of every world, its inputs the Data fields the earlier stages wrote and its outputs written
 * back (dense-path models; round 6).  `stage` (MJW_STAGE_*) names the reference function it replaces:
 *   1 kinematics          smooth.py:357-415   (qpos, mocap -> body / joint / geom / site frames)
 *   2 com_pos             smooth.py:601-632   (frames -> subtree_com, cinert, cdof)
 *   3 camlight            smooth.py:635-803   (frames, subtree_com -> camera / light frames)
 *   4 tendon              smooth.py:3627-3700 (qpos, frames -> ten_length, ten_J)
 *   5 crb                 smooth.py:888-912   (cinert, cdof -> crb, qM incl. armature)
 *   6 make_constraint     constraint.py:2718-2779 (contacts in d.contact + frames -> efc rows)
 *   7 transmission        smooth.py:2605-2700 (actuator_length / moment; not for BODY transmissions)
 *   8 com_vel             smooth.py:1935-2038 (+ actuator_velocity, forward.py:540-562)
 *   9 passive             passive.py:535-563
 *  10 rne                 smooth.py:1276-1300 (flg_acc = False; + tendon_bias, :1878-1932) */
enum { MJW_STAGE_KINEMATICS = 1, MJW_STAGE_COM_POS = 2, MJW_STAGE_CAMLIGHT = 3, MJW_STAGE_TENDON = 4, MJW_STAGE_CRB = 5,
       MJW_STAGE_MAKE_CONSTRAINT = 6, MJW_STAGE_TRANSMISSION = 7, MJW_STAGE_COM_VEL = 8, MJW_STAGE_PASSIVE = 9, MJW_STAGE_RNE = 10 };
int mjw_stage(const mjw_model_t* m, const mjw_data_t* d, int stage, void* stream);
/* sensors of the stages in `stages` (bit 0: sensor_pos, sensor.py:761; bit 1: sensor_vel, :1377;
 * bit 2: sensor_acc with rne_postconstraint, :2447) from the Data of the current step; mjw_step /
 * mjw_forward run all three themselves, the stage entry points above run none */
int mjw_sensor(const mjw_model_t* m, const mjw_data_t* d, int stages, void* stream);
/* Runge-Kutta 4 (forward.py:457-491 rungekutta4): expects `forward` to have run on the current state
 * (mjw_step does this itself for RK4 models); runs three more forward passes and advances the state.
 * The t0 copies and the weighted sums live in the Data workspace fields qpos_t0 ... act_dot_rk. */
int mjw_rungekutta4(const mjw_model_t* m, const mjw_data_t* d, void* stream);
/* one RK4 bookkeeping op, for hosts that run `forward` themselves between them (Python callbacks):
 * op 0 = save t0 and accumulate B[0] (scale), 1 = _rk_perturb_state (forward.py:357-399),
 * 2 = _rk_accumulate (:402-454), 3 = restore t0 and _advance (:484-491, :213-274) */
int mjw_rk4_op(const mjw_model_t* m, const mjw_data_t* d, int op, float scale, void* stream);
/* per-step control noise (Ornstein-Uhlenbeck + Halton) of the reference benchmark;
 * center: device float[nu] or NULL; world ids are d->world_offset + local id */
/* Device self-checks of the wave primitives of the dense path (no reference counterpart):
 * which = 0: in = n x 64 floats, out[w] = sum of chunk w, out[n + 64w + l] = in[64w + l] + in[64w + (l^32)];
 * which = 1: in = n row-major 32x32 SPD matrices, out = their inverses (Cholesky + MFMA X^T X). */
int mjw_selftest(int which, const float* in, float* out, int n, void* stream);
/* Device replay of the reference's collision known-answer tests (csrc/mjw_kat.hip, tests/test_gpu_golden.py):
 * which = 0: ccd() as collision_gjk_test.py:34-265 `_geom_dist` calls it (+ box multi-contact), one record of
 *            48 floats per case in `in`, aux = {max ccd_iterations, mesh vertices...}, 8 floats out per case;
 * which = 1: sphere / capsule / box / cylinder vs triangle (collision_primitive_core_test.py), 32 floats in,
 *            16 out per case, aux unused. */
int mjw_kat(int which, const float* in, const float* aux, float* out, int n, void* stream);

/* qfrc_actuator from the Data's actuator_force and moment rows (forward.py:899-927), for hosts that run
 * the act_dyn / act_gain / act_bias callbacks (forward.py:876-881) between mjw_fwd_actuation and the
 * moment map; dense path only */
int mjw_actuator_map(const mjw_model_t* m, const mjw_data_t* d, void* stream);

int mjw_ctrl_noise(const mjw_model_t* m, const mjw_data_t* d, const float* center, int step, float std, float rate,
                   void* stream);

/* The collision sub-stages (mujoco_warp/__init__.py:33-35) over the reference's CollisionContext arrays
 * (collision_core.py:345-365), each `naconmax` long: collision_pair (2 ints, type-ordered geoms),
 * collision_pairid (2 ints: explicit <pair> id or -1 / -2 excluded, collision-sensor id or -1),
 * collision_worldid.  Both read the geom frames d.geom_xpos / d.geom_xmat of the position stage.
 * mjw_nxn_broadphase replaces nxn_broadphase (collision_driver.py:697-731): survivors of
 * opt_broadphase_filter over the filtered NXN list, counted in d.ncollision (which the caller zeroes), slots
 * past naconmax dropped.  mjw_sap_broadphase replaces sap_broadphase (:554-643): bounding spheres projected on
 * the reference's fixed direction and sorted per world (ngeom <= 4096), the sweep's candidates (_sap_range
 * :421-441) that are NXN pairs through the same filter, appended the same way (round 6; ABI 34).
 * mjw_primitive_narrowphase replaces primitive_narrowphase (collision_primitive.py:1461-1549): contacts of
 * the candidates [0, min(ncollision, naconmax)) whose type pair (t1 <= t2) has bit 8 t1 + t2 set in
 * typemask, appended to the contact pool at d.nacon as write_contact does (collision_core.py:160-232). */
int mjw_nxn_broadphase(const mjw_model_t* m, const mjw_data_t* d, int* collision_pair, int* collision_pairid, int* collision_worldid,
                       void* stream);
int mjw_sap_broadphase(const mjw_model_t* m, const mjw_data_t* d, int* collision_pair, int* collision_pairid, int* collision_worldid,
                       void* stream);
int mjw_primitive_narrowphase(const mjw_model_t* m, const mjw_data_t* d, const int* collision_pair, const int* collision_pairid,
                              const int* collision_worldid, unsigned long long typemask, void* stream);

/* Batched ray casting (ray.py:1212-1312 `rays` without a render context; ABI 35): for every world and ray the
 * nearest geom along pnt + x vec, x >= 0, over all geom types at the frames d.geom_xpos / d.geom_xmat of
 * the last position stage (no kinematics run here).  pnt / vec: device float (nb, nray, 3) with nb = 1 or
 * d->nworld (world w reads row w % nb); vec is not normalised and dist is in units of |vec|.  geomgroup: six
 * host ints or NULL (all -1 or NULL: no group filter, else geoms with geomgroup[clamp(geom_group, 0, 5)] == 0
 * are skipped); flg_static == 0 skips geoms of bodies welded to the world; bodyexclude: device int (nray,),
 * geoms of that body are skipped (-1: none).  Geoms with alpha 0 (their material's when they have one, else
 * their own) are skipped.  Outputs, device: dist (nworld, nray), geomid (nworld, nray), normal (nworld, nray, 3);
 * a miss gives -1, -1, 0; equal distances go to the lowest geom id.  nray == 0 is a successful no-op. */
int mjw_rays(const mjw_model_t* m, const mjw_data_t* d, const mjw_ray_model_t* rm, const float* pnt, int pnt_nb, const float* vec,
             int vec_nb, int nray, const int* geomgroup, int flg_static, const int* bodyexclude, float* dist, int* geomid,
             float* normal, void* stream);

/* Batched camera rendering (render.py `render`): one launch writes, for every world, the segmentation (geom id,
 * -1 background), planar depth (distance along the optical axis, 0 background) and shaded RGB (packed, background
 * (25, 25, 51, 255)) images of the context's cameras, from the camera / light / geom frames of the last position stage
 * (no kinematics run here).  The pixel rays are made in the kernel (render_util.py:67-125) from cam_fovy /
 * cam_sensorsize / cam_intrinsic, which are read per world (row w % nb).  A geom is drawn iff its group is a bit of
 * rc->group_mask (no alpha, static or body rule); the nearest hit is found by the geom loop of mjw_rays.  Shading:
 * hemispheric ambient plus the active lights, with one any-hit shadow pass per castshadow light when use_shadows.
 * A successful no-op for d->nworld <= 0 or rc->ntile == 0; null arguments give -1, a ray model whose ngeom differs
 * -4, more workgroups than the grid holds -2. */
int mjw_render(const mjw_model_t* m, const mjw_data_t* d, const mjw_ray_model_t* rm, const mjw_render_t* rc, void* stream);

/* mjw_rays / mjw_render with the meshes walked through the BVHs of `bvh` in place of the loop over every face; the
 * results are those of mjw_rays / mjw_render.  The trees were built from the unbatched mesh_vert: with a per-world
 * mesh_vert (mesh_vert_nb > 1), and for a model without mesh faces, the call is mjw_rays / mjw_render.  A null bvh
 * or null tables give -1; counts that differ from the model's, a leaf_size above 4 or a max_depth above 32 give -4. */
int mjw_rays_bvh(const mjw_model_t* m, const mjw_data_t* d, const mjw_ray_model_t* rm, const float* pnt, int pnt_nb, const float* vec,
                 int vec_nb, int nray, const int* geomgroup, int flg_static, const int* bodyexclude, float* dist, int* geomid,
                 float* normal, const mjw_bvh_t* bvh, void* stream);
int mjw_render_bvh(const mjw_model_t* m, const mjw_data_t* d, const mjw_ray_model_t* rm, const mjw_render_t* rc, const mjw_bvh_t* bvh,
                   void* stream);

/* Inverse dynamics at the caller's acceleration (inverse.py `inverse`, its constraint and combine steps; ABI 36):
 * with the position and velocity stages of the current state in `d` (qM, qfrc_bias, qfrc_passive and the constraint
 * rows), one launch evaluates the row law once at d->qacc, which it only reads.  Over the rows r < n = min(nefc, njmax):
 * Jaref = J qacc - aref, efc_force and efc_state from the row law (equality, friction loss, limit, frictionless,
 * pyramidal and elliptic rows; an elliptic contact whose rows njmax cuts contributes nothing), then
 * qfrc_constraint = J' efc_force, efc_Ma = M qacc and
 * qfrc_inverse = qfrc_bias + efc_Ma - qfrc_passive - qfrc_constraint.  Rows r >= n of efc_force / efc_state are left
 * alone; without rows (njmax == 0, the constraint disable flag, no active row) qfrc_constraint is exactly zero.
 * Sparse models also use sp_row and the transposed-index workspace (efc_JT_*, sp_idx16, sp_cnt), as mjw_solve does.
 * nworld <= 0 is a successful no-op without a launch; null model / data / arrays give -1, a dense-path model with
 * nv > 64 gives -2. */
int mjw_inverse(const mjw_model_t* m, const mjw_data_t* d, void* stream);

/* Constraint islands (island.py `island`, MuJoCo's mj_island): which kinematic trees the active constraint rows of
 * each world couple.  It stays out of mjw_model_t / mjw_data_t like mjw_ray_model_t: the tree ids and the four
 * outputs, every pointer a device pointer. */
typedef struct mjw_island_t {
  int32_t ntree;   /* must equal mjw_model_t.ntree */
  int32_t pad_;
  const int32_t* body_treeid;  /* (nbody,) -1: static */
  const int32_t* dof_treeid;   /* (nv,) */
  int32_t* nisland;            /* (nworld,) */
  int32_t* tree_island;        /* (nworld, ntree) */
  int32_t* dof_island;         /* (nworld, nv) */
  int32_t* efc_island;         /* (nworld, njmax) */
} mjw_island_t;
int mjw_sizeof_island(void);
/* trees per world up to which the launch keeps its union-find in LDS; above it the world's tree_island / dof_island
 * rows are the scratch (same results) */
int mjw_island_lds_trees(void);
/* One launch, one workgroup per world, over the rows r < n = min(nefc, njmax) the last position stage left.  The trees
 * of a row: connect / weld rows the trees of their two bodies (through site_bodyid with site semantics), dof friction
 * rows dof_treeid[efc_id], joint limit rows dof_treeid[jnt_dofadr[efc_id]], contact rows with two geoms the trees of
 * the geoms' bodies (efc_id: the contact's pool slot), every other row (joint / tendon / flex equalities, tendon
 * friction and limits, contacts with a flex side) dof_treeid of the dofs with a non-zero entry in its row of efc_J
 * (either layout); tree ids < 0 are dropped, an id outside its array contributes nothing.  Islands are the connected
 * components of the trees some row touches, numbered in ascending order of their smallest tree (the reference's
 * upper-triangle edges of generic rows lose components; this does not).  Writes nisland, tree_island (-1:
 * unconstrained), dof_island = tree_island[dof_treeid] and efc_island (the island of the row's trees, -1 for a row
 * without trees and for every r >= n) and nothing else; allocates nothing (graph capturable).  ntree == 0 zeroes
 * nisland without a launch; nworld <= 0 is a successful no-op; null arguments give -1, an ntree that differs from
 * the model's -4. */
int mjw_island(const mjw_model_t* m, const mjw_data_t* d, const mjw_island_t* is, void* stream);

/* Flex rendering (mjw_flex_refit, mjw_render_flex): the host-built tables of a render context made with
 * render_flex, and its two per-world buffers.  It stays out of mjw_model_t / mjw_render_t like mjw_island_t; every
 * pointer is a device pointer and every vertex / element / edge id in the tables is global (flex_vertadr /
 * flex_elemadr / flex_edgeadr already added), so the kernels need none of the model's flex tables besides these.
 * info: 12 ints per flex: flex_dim, flex_vertadr, flex_vertnum, first face, faces, first node, nodes, tree depth,
 * first entry of level, flex_edgeadr, flex_edgenum, 0.  Faces (dim 2: two per element, then two per boundary
 * fragment; dim 3: the flex_shell triangles; dim 1: none, its edges are capsules) are corner records: three per
 * face, each (vertex, sign, source): the point is xpos[vertex] + sign * flex_radius * n with n the vertex normal
 * (source < 0) or the flat normal of element `source`; sign 0 is the vertex itself.  node / tri: one tree per
 * flex over its faces in the layout of mjw_bvh_t (face ids local to the flex); the boxes in `node` are the rest
 * pose's and only its two ints are read.  level: per tree depth + 1 local node indices, the first node of each
 * level and the node count.  node_box row w: the boxes of all nodes as mjw_flex_refit left them, then one box per
 * flex around its vertices grown by the radius. */
typedef struct mjw_flexrender_t {
  int32_t nflex;       /* must equal mjw_model_t.nflex */
  int32_t nflexvert;   /* must equal mjw_model_t.nflexvert */
  int32_t nflexelem;   /* must equal mjw_model_t.nflexelem */
  int32_t nflexedge;   /* must equal mjw_model_t.nflexedge */
  int32_t nface;       /* faces of all flexes: rows of corner / 3, entries of tri */
  int32_t nnode;       /* nodes of all trees */
  int32_t ninc;        /* entries of inc */
  int32_t nlevel;      /* entries of level */
  int32_t leaf_size;   /* faces per leaf at the most; at most 4 */
  int32_t max_depth;   /* levels of the deepest tree; at most 32 */
  int32_t min_faces;   /* flexes with fewer faces are intersected by the loop over their faces (same results) */
  int32_t pad_;
  const int32_t* info;        /* (nflex, 12) */
  const float* flex_radius;   /* (nflex,) */
  const float* flex_rgba;     /* (nflex, 4) */
  const int32_t* corner;      /* (nface, 3, 3) */
  const int32_t* elem_vert;   /* (nflexelem, 3) the vertices of the dim-2 elements (flex_elem) */
  const int32_t* edge_vert;   /* (nflexedge, 2) flex_edge */
  const int32_t* inc_adr;     /* (nflexvert + 1,) vertex -> incident dim-2 elements, ascending: a CSR */
  const int32_t* inc;         /* (ninc,) */
  const float* node;          /* (nnode, 8) */
  const int32_t* tri;         /* (nface,) */
  const int32_t* level;       /* (nlevel,) */
  float* node_box;            /* (nworld, nnode + nflex, 6) minimum, maximum */
  float* vert_norm;           /* (nworld, nflexvert, 3) vertex normals of the dim-2 flexes */
} mjw_flexrender_t;
int mjw_sizeof_flexrender(void);
/* Refits every flex tree of every world to d->flexvert_xpos: one launch, one workgroup per (world, flex): the vertex
 * normals of a dim-2 flex (the normalised sum of its incident elements' unit normals in ascending element order; a
 * zero sum stays zero), every leaf's box as the exact float32 minimum / maximum of its faces' points, the inner
 * nodes level by level from the deepest up, and the whole-flex box.  Writes fr->node_box and fr->vert_norm and
 * nothing else; no atomics, graph capturable.  nflex == 0 or nworld <= 0 is a successful no-op; null arguments or
 * tables give -1; counts that differ from the model's, a leaf_size above 4 or a max_depth above 32 give -4; more
 * workgroups than the grid holds -2. */
int mjw_flex_refit(const mjw_model_t* m, const mjw_data_t* d, const mjw_flexrender_t* fr, void* stream);
/* mjw_render_bvh (bvh != NULL) or mjw_render (bvh == NULL: the meshes' faces are looped over) with the flexes of
 * `fr` drawn as well, from the boxes and normals the last mjw_flex_refit left: it does not refit.  The nearest hit
 * over geoms and flexes; a flex replaces a geom only when strictly nearer, the lower flex id and within a flex the
 * lower face id win ties.  A flex pixel has segmentation -2, the colour flex_rgba and, on a triangle, the winding
 * normal turned to face the ray; flexes throw and receive shadows like geoms.  Flexes of at least min_faces faces
 * are walked through their tree, smaller ones face by face, with the same images bit for bit.  With nflex == 0 it
 * is mjw_render_bvh / mjw_render.  Errors as those calls and mjw_flex_refit. */
int mjw_render_flex(const mjw_model_t* m, const mjw_data_t* d, const mjw_ray_model_t* rm, const mjw_render_t* rc, const mjw_bvh_t* bvh,
                    const mjw_flexrender_t* fr, void* stream);

/* Textured rendering (mjw_render_tex): the 2D textures of a render context made with use_textures, the materials'
 * texture ids and repeats (per world: world w reads row w % nb) and the meshes' texture coordinates.  It stays out
 * of mjw_model_t / mjw_render_t like mjw_flexrender_t; every pointer is a device pointer.  tex_data: one word per
 * texel, r | g << 8 | b << 16 | 255 << 24, row y of a texture is v; tex_adr: the first word of each texture, -1 for
 * one that is never sampled (cube, skybox, no data).  mesh_facetexcoord indexes mesh_texcoord relative to
 * mesh_texcoordadr[mesh], which is -1 for a mesh without texture coordinates.  The kernel treats every id or
 * address outside its table as "no texture": a table that does not fit samples nothing and nothing outside it is read. */
typedef struct mjw_texture_t {
  int32_t ntex;              /* textures: entries of tex_adr / tex_width / tex_height */
  int32_t ntexdata;          /* words of tex_data */
  int32_t nmat;              /* must equal mjw_ray_model_t.nmat */
  int32_t nmesh;             /* entries of mesh_texcoordadr: the model's nmesh, or 0 */
  int32_t ntexcoord;         /* rows of mesh_texcoord */
  int32_t nmeshface;         /* rows of mesh_facetexcoord: mjw_ray_model_t.nmeshface, or 0 */
  int32_t mat_texid_nb;      /* >= 1 */
  int32_t mat_texrepeat_nb;  /* >= 1 */
  const int32_t* mat_texid;         /* (mat_texid_nb, nmat, 10): texture id per role; only role 1 (RGB) is read */
  const float* mat_texrepeat;       /* (mat_texrepeat_nb, nmat, 2) */
  const int32_t* tex_data;          /* (ntexdata,) */
  const int32_t* tex_adr;           /* (ntex,) */
  const int32_t* tex_width;         /* (ntex,) */
  const int32_t* tex_height;        /* (ntex,) */
  const float* mesh_texcoord;       /* (ntexcoord, 2) */
  const int32_t* mesh_texcoordadr;  /* (nmesh,) */
  const int32_t* mesh_facetexcoord; /* (nmeshface, 3) */
} mjw_texture_t;
int mjw_sizeof_texture(void);
/* mjw_render_flex (fr != NULL), mjw_render_bvh (fr == NULL, bvh != NULL) or mjw_render (both NULL) with the base
 * colour of every geom pixel multiplied, before the ambient and light terms, by a bilinear sample of the texture
 * that role 1 of the geom's material names, where the geom is a plane (uv = the hit in the geom's frame, x and y)
 * or a mesh whose mesh has texture coordinates (uv = the barycentric mean of the hit face's three; the face is the
 * nearest, the lowest id among equal distances).  s = frac(uv * texrepeat); the four texels around (s.x W - 0.5,
 * s.y H - 0.5) are blended with float32 weights, indices taken modulo W and H.  Every other geom, a mesh without
 * texture coordinates and every flex keep their colour; depth and segmentation are those of the call without
 * textures.  With ntex, ntexdata or nmat zero it is that call.  Errors as those calls; a null tex or a null table
 * with a non-zero count gives -1, a negative count, a batch size under 1 or counts that differ from the model's -4. */
int mjw_render_tex(const mjw_model_t* m, const mjw_data_t* d, const mjw_ray_model_t* rm, const mjw_render_t* rc, const mjw_bvh_t* bvh,
                   const mjw_flexrender_t* fr, const mjw_texture_t* tex, void* stream);

/* Finite-difference linearisation of the step (MuJoCo's mjd_transitionFD): x' ~ A dx + B du, sensordata ~ C dx + D du,
 * in the tangent space dx = [dq (nv), dv (nv), dact (na)], ndx = 2 nv + na, with K = ndx + nu input columns (the state
 * columns, then ctrl).  Every perturbed copy of a world is one more world of a scratch Data: slot c of world w is
 * scratch world c * nworld + w, slot 0 holds the nominal state, slots 1 .. ncp the + nudges of the pass's columns
 * col0 .. col0 + ncols - 1, and with `centered` slots 1 + ncp .. 2 ncp their - nudges, where ncp is the columns a pass
 * holds: ncol_pass = 1 + 2 ncp centred, 1 + ncp forward.  mjw_fd_perturb fills the slots, the caller steps the
 * scratch Data, mjw_fd_difference turns the stepped slots into the pass's columns of A..D.  The struct holds the
 * pointers of the nominal Data's (n_*) and the scratch Data's (s_*) fields so that the kernels do not take two
 * mjw_data_t by value; every pointer is a device pointer, an array of zero size may be null.
 *
 * The ctrl columns follow MuJoCo's range rule for an actuator with actuator_ctrllimited while CLAMPCTRL is not
 * disabled: the + nudge is made only if ctrl and ctrl + eps lie inside ctrlrange, the - nudge only if `centered` or the
 * + nudge was impossible, and ctrl - eps and ctrl lie inside; the column is then centred, forward, backward or zero,
 * per world.  A forward context keeps the - nudge of such a column in the column's one slot.  A slot whose nudge is
 * not made, and every slot past the pass's ncols columns, holds the nominal state. */
typedef struct mjw_fd_t {
  int32_t nworld;     /* worlds of the nominal Data; the scratch Data holds ncol_pass * nworld */
  int32_t ncol;       /* K = 2 nv + na + nu, checked against the model */
  int32_t ncol_pass;  /* slots per world */
  int32_t centered;   /* 0 / 1 */
  int32_t col0;       /* first column of this pass */
  int32_t ncols;      /* columns of this pass, 1 .. ncp */
  const float* n_time;            /* (nworld,) */
  const float* n_qpos;            /* (nworld, nq) */
  const float* n_qvel;            /* (nworld, nv) */
  const float* n_act;             /* (nworld, na) */
  const float* n_ctrl;            /* (nworld, nu) */
  const float* n_qacc_warmstart;  /* (nworld, nv) */
  const float* n_qfrc_applied;    /* (nworld, nv) */
  const float* n_xfrc_applied;    /* (nworld, nbody, 6) */
  const float* n_mocap_pos;       /* (nworld, nmocap, 3) */
  const float* n_mocap_quat;      /* (nworld, nmocap, 4) */
  const int32_t* n_eq_active;     /* (nworld, neq) */
  float* s_time;                  /* the same fields of the scratch Data, (ncol_pass * nworld, ...) */
  float* s_qpos;
  float* s_qvel;
  float* s_act;
  float* s_ctrl;
  float* s_qacc_warmstart;
  float* s_qfrc_applied;
  float* s_xfrc_applied;
  float* s_mocap_pos;
  float* s_mocap_quat;
  int32_t* s_eq_active;
  const float* s_sensordata;      /* (ncol_pass * nworld, nsensordata); read by mjw_fd_difference when C is given */
  float* A;                       /* (nworld, ndx, lda) */
  float* B;                       /* (nworld, ndx, ldb); unused when nu == 0 */
  float* C;                       /* (nworld, nsensordata, ldc) or null (then D is null too) */
  float* D;                       /* (nworld, nsensordata, ldd); unused when nu == 0 */
  int64_t lda, ldb, ldc, ldd;     /* floats between consecutive rows: >= ndx, nu, ndx, nu */
} mjw_fd_t;
int mjw_sizeof_fd(void);
/* Fills every slot of the scratch Data: one wave per scratch world copies, bitwise, the world's time, qpos, qvel,
 * act, ctrl, qacc_warmstart, qfrc_applied, xfrc_applied, eq_active, mocap_pos and mocap_quat; then one lane applies
 * the slot's nudge.  Column k < nv nudges the position in the tangent space (slide, hinge, free translation: add
 * +-eps; free rotation and ball: quat <- normalize(quat * exp(+-eps e)), the rotation vector in the local frame, as
 * mj_integratePos), the next nv columns add to qvel, the next na to act, the last nu to ctrl under the range rule.
 * `d` is the nominal Data and is only read; A..D are not used.  Allocates nothing, no atomics (graph capturable).
 * nworld <= 0 is a successful no-op; null arguments or arrays give -1; nv == 0, eps <= 0, sizes that differ from the
 * model's or the Data's, or a column range outside 0 .. K give -4. */
int mjw_fd_perturb(const mjw_model_t* m, const mjw_data_t* d, const mjw_fd_t* fd, float eps, void* stream);
/* Writes the pass's columns of A, B (and C, D when given) from the stepped slots: one workgroup per (world, tile of
 * columns) stages the differences of the slots' qpos, qvel, act and sensordata in LDS (rows padded to an odd stride)
 * and stores them with lanes along the last dimension.  With h = 2 eps for a centred column (y- to y+) and eps for a
 * one-sided one (nominal to +, or - to nominal), position rows are mj_differentiatePos (scalar joints and free
 * translation (q2 - q1) / h; quaternions log(conj(q1) * q2) / h, the angle in (-pi, pi], once per column and joint),
 * every other row (y2 - y1) / h, a true division; a column without a nudge is zero.  Writes rows 0 .. ndx - 1
 * (nsensordata - 1) of columns col0 .. col0 + ncols - 1 and nothing else.  Errors as mjw_fd_perturb; more rows than
 * one column's staging holds (2 nv + na + nsensordata > 12287) give -2. */
int mjw_fd_difference(const mjw_model_t* m, const mjw_data_t* d, const mjw_fd_t* fd, float eps, void* stream);

#ifdef __cplusplus
}
#endif
#endif
