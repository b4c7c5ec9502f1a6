// vq_pass1_d64.hip -- the pass-1 kernels of D = 64 with the per-tile seed piece (no RES: any number of code tiles) (dvq_pass1.h),
// instantiated and launched here.
#include "dvq_pass1.h"

int dvq_launch_pass1_d64(const P1Plan &p, const P1Args &a) { return launch_pass1_res<64, false>(p, a); }
#ifdef DVQ_TUNING
int dvq_tuning_set_pass1_d64(void *stamps, void *tokdbg) { return dvq_tuning_set_unit(stamps, tokdbg); }
#endif
