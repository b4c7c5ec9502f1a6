// vq_pass1_d64_res.hip -- the pass-1 kernels of D = 64 with the resident seed table (RES: at most 32 code tiles per workgroup) (dvq_pass1.h),
// instantiated and launched here.
#include "dvq_pass1.h"

int dvq_launch_pass1_d64_res(const P1Plan &p, const P1Args &a) { return launch_pass1_res<64, true>(p, a); }
#ifdef DVQ_TUNING
int dvq_tuning_set_pass1_d64_res(void *stamps, void *tokdbg) { return dvq_tuning_set_unit(stamps, tokdbg); }
#endif
