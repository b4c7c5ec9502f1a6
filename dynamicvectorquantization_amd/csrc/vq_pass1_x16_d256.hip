// vq_pass1_x16_d256.hip -- pass 1 on 16-bit latents (fp16 and bf16; dense, lane per token) at D = 256 with the per-tile seed piece (dvq_pass1.h),
// instantiated and launched here.
#include "dvq_pass1.h"

int dvq_launch_pass1_x16_d256(const P1Plan &p, const P1Args &a) { return launch_pass1_x16<256, false>(p, a); }
