// lsi_fused with the regularized l-QR (lqr_wave_body<41,12,REG>): nVar <= 40, level dims <= 12
#include "lsi_fused_impl.h"
LEXLS_LSI_FUSED_INSTANCE_REG(launch_lsi_fused_41x12_R, 41, 12, false)
