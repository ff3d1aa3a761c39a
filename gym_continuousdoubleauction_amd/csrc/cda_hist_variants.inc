// cda_hist_variants.inc - the ONE place that knows the compiled history depths of the policy network (include/cda_mlp.h CDA_MLP_HIST_VARIANTS beside the default 4).
// Including this file includes  CDA_HIST_BODY  (a file name) once per depth, the default depth 4 first, between the includer's  CDA_HIST_OPEN  and  CDA_HIST_CLOSE
// (e.g. a namespace; may be empty), with  CDA_MLP_HIST = the depth  (include/cda_mlp.h's layout macros follow it) and  CDA_HIST_SFX(x) = x with the depth's suffix:
// x itself at depth 4, x_h<H> at the others.  Afterwards CDA_MLP_HIST is 4 again.  No include guard on purpose; the list of the depths is defined once.
#ifndef CDA_HIST_DEPTHS
#define CDA_HIST_DEPTHS(X) X(1) X(2) X(3) X(6) X(7) X(8)       // the depths beside 4: X(h) once each (what a switch over n_hist is generated from)
#define CDA_HIST_PASTE(x, h) x##_h##h
#define CDA_HIST_PASTE2(x, h) CDA_HIST_PASTE(x, h)
#endif
#undef CDA_MLP_HIST
#define CDA_MLP_HIST 4
#define CDA_HIST_SFX(x) x
CDA_HIST_OPEN
#include CDA_HIST_BODY
CDA_HIST_CLOSE
#undef CDA_HIST_SFX
#define CDA_HIST_SFX(x) CDA_HIST_PASTE2(x, CDA_MLP_HIST)
#undef CDA_MLP_HIST
#define CDA_MLP_HIST 1
CDA_HIST_OPEN
#include CDA_HIST_BODY
CDA_HIST_CLOSE
#undef CDA_MLP_HIST
#define CDA_MLP_HIST 2
CDA_HIST_OPEN
#include CDA_HIST_BODY
CDA_HIST_CLOSE
#undef CDA_MLP_HIST
#define CDA_MLP_HIST 3
CDA_HIST_OPEN
#include CDA_HIST_BODY
CDA_HIST_CLOSE
#undef CDA_MLP_HIST
#define CDA_MLP_HIST 6
CDA_HIST_OPEN
#include CDA_HIST_BODY
CDA_HIST_CLOSE
#undef CDA_MLP_HIST
#define CDA_MLP_HIST 7
CDA_HIST_OPEN
#include CDA_HIST_BODY
CDA_HIST_CLOSE
#undef CDA_MLP_HIST
#define CDA_MLP_HIST 8
CDA_HIST_OPEN
#include CDA_HIST_BODY
CDA_HIST_CLOSE
#undef CDA_HIST_SFX
#undef CDA_MLP_HIST
#define CDA_MLP_HIST 4
