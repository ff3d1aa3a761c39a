/* cda_mlp_variant.h - one object file of csrc/cda_mlp.hip per history depth and hidden activation.
 *
 * The network kernels are compiled for ONE observation width (CDA_MLP_HIST frames of 42 floats: layer 1's k-steps, W1's operand layout, the LDS tiles, the dW1 slab
 * are compile-time shapes) and ONE hidden activation (CDA_MLP_ACT: 0 tanh, 1 relu, 2 elu, 3 linear - csrc/cda_mlp_dev.inc ActT).  The default build (CDA_MLP_HIST = 4,
 * the reference's n_hist; tanh) defines the entry points of include/cda_mlp.h under their own names; a build with -DCDA_MLP_HIST=<H> and / or -DCDA_MLP_ACT=<a>
 * renames every one of them to <name>[_h<H>][_<act>] (cda_mlp_forward_relu, cda_mlp_forward_h6_elu) BEFORE the header is read, so declarations and definitions
 * agree and the objects link into one library (__graft_entry__.build_hip compiles CDA_MLP_HIST_VARIANTS x CDA_MLP_ACT_VARIANTS).  Entry points that depend on
 * neither (the permutation, the unfused loss, GAE, episode returns, league assignment) are not here: include/cda_learner.h declares them, csrc/cda_learner.hip is
 * compiled once and they are never renamed.  Generated list: EVERY function include/cda_mlp.h itself declares, and nothing else (tests/test_capi_load.py checks it).
 * -DCDA_MLP_VFS=1 builds the shared-trunk network (RLlib's vf_share_layers: the value head reads the policy half, the value half is dead) and appends _vfs behind
 * the other suffixes: <name>[_h<H>][_<act>]_vfs (cda_mlp_forward_vfs, cda_mlp_forward_backward_h6_elu_vfs). */
#ifndef CDA_MLP_VARIANT_H
#define CDA_MLP_VARIANT_H
#if defined(CDA_MLP_ACT) && CDA_MLP_ACT == 1
#define CDA_MLP_ACT_NAME relu
#elif defined(CDA_MLP_ACT) && CDA_MLP_ACT == 2
#define CDA_MLP_ACT_NAME elu
#elif defined(CDA_MLP_ACT) && CDA_MLP_ACT == 3
#define CDA_MLP_ACT_NAME linear
#elif defined(CDA_MLP_ACT) && CDA_MLP_ACT != 0
#error "CDA_MLP_ACT: 0 tanh, 1 relu, 2 elu, 3 linear"
#endif
#define CDA_MLP_SFX2(n, h) n##_h##h
#define CDA_MLP_SFX1(n, h) CDA_MLP_SFX2(n, h)
#define CDA_MLP_ASFX2(n, a) n##_##a
#define CDA_MLP_ASFX1(n, a) CDA_MLP_ASFX2(n, a)
#if defined(CDA_MLP_HIST) && CDA_MLP_HIST != 4 && defined(CDA_MLP_ACT_NAME)
#define CDA_MLP_BSFX(n) CDA_MLP_ASFX1(CDA_MLP_SFX1(n, CDA_MLP_HIST), CDA_MLP_ACT_NAME)
#elif defined(CDA_MLP_HIST) && CDA_MLP_HIST != 4
#define CDA_MLP_BSFX(n) CDA_MLP_SFX1(n, CDA_MLP_HIST)
#elif defined(CDA_MLP_ACT_NAME)
#define CDA_MLP_BSFX(n) CDA_MLP_ASFX1(n, CDA_MLP_ACT_NAME)
#endif
#ifndef CDA_MLP_VFS
#define CDA_MLP_VFS 0
#endif
#define CDA_MLP_VSFX2(n) n##_vfs
#define CDA_MLP_VSFX1(n) CDA_MLP_VSFX2(n)
#if CDA_MLP_VFS && defined(CDA_MLP_BSFX)
#define CDA_MLP_SFX(n) CDA_MLP_VSFX1(CDA_MLP_BSFX(n))
#elif CDA_MLP_VFS
#define CDA_MLP_SFX(n) CDA_MLP_VSFX1(n)
#elif defined(CDA_MLP_BSFX)
#define CDA_MLP_SFX(n) CDA_MLP_BSFX(n)
#endif
#ifdef CDA_MLP_SFX
#define cda_mlp_tile_rows CDA_MLP_SFX(cda_mlp_tile_rows)
#define cda_mlp_wgrad_jobs CDA_MLP_SFX(cda_mlp_wgrad_jobs)
#define cda_mlp_pack CDA_MLP_SFX(cda_mlp_pack)
#define cda_mlp_policy_step CDA_MLP_SFX(cda_mlp_policy_step)
#define cda_mlp_policy_act CDA_MLP_SFX(cda_mlp_policy_act)
#define cda_mlp_forward CDA_MLP_SFX(cda_mlp_forward)
#define cda_mlp_prep_rows CDA_MLP_SFX(cda_mlp_prep_rows)
#define cda_mlp_forward_train CDA_MLP_SFX(cda_mlp_forward_train)
#define cda_mlp_backward CDA_MLP_SFX(cda_mlp_backward)
#define cda_mlp_wgrad CDA_MLP_SFX(cda_mlp_wgrad)
#define cda_mlp_adam CDA_MLP_SFX(cda_mlp_adam)
#define cda_mlp_reduce CDA_MLP_SFX(cda_mlp_reduce)
#define cda_mlp_apply CDA_MLP_SFX(cda_mlp_apply)
#define cda_mlp_rollout_chain CDA_MLP_SFX(cda_mlp_rollout_chain)
#define cda_mlp_values CDA_MLP_SFX(cda_mlp_values)
#define cda_mlp_values_counted CDA_MLP_SFX(cda_mlp_values_counted)
#define cda_mlp_forward_backward CDA_MLP_SFX(cda_mlp_forward_backward)
#define cda_mlp_league_step CDA_MLP_SFX(cda_mlp_league_step)
#define cda_mlp_league_rollout_chain CDA_MLP_SFX(cda_mlp_league_rollout_chain)
#define cda_mlp_league_act CDA_MLP_SFX(cda_mlp_league_act)
#define cda_mlp_eval_chain CDA_MLP_SFX(cda_mlp_eval_chain)
#define cda_mlp_league_eval_chain CDA_MLP_SFX(cda_mlp_league_eval_chain)
#define cda_mlp_selftest_mfma CDA_MLP_SFX(cda_mlp_selftest_mfma)
#endif
#endif
