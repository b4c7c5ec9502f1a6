// vq_pass1_x16_d256_res.hip -- pass 1 on 16-bit latents (fp16 and bf16; dense, lane per token) at D = 256 with the resident seed table (RES: at most 32 code tiles per workgroup) (dvq_pass1.h),
// instantiated and launched here.
#include "dvq_pass1.h"

int dvq_launch_pass1_x16_d256_res(const P1Plan &p, const P1Args &a) { return launch_pass1_x16<256, true>(p, a); }
