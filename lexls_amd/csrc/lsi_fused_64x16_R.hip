// lsi_fused with the regularized l-QR (lqr_wave_body<64,16,REG>): nVar <= 63, level dims <= 16
#include "lsi_fused_impl.h"
LEXLS_LSI_FUSED_INSTANCE_REG(launch_lsi_fused_64x16_R, 64, 16, false)
