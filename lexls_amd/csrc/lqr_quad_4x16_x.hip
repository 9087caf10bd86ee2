#include "lqr_quad_impl.h"
LEXLS_QUAD_INSTANCE(launch_quad_4x16_x, 4, 16, false, 0)
