// x only, indirect: the accuracy guard's bit-exact re-solve of the problems lqr_qtol flagged (same arithmetic as lqr_quad_3x12s7_x)
#include "lqr_quad_impl.h"
LEXLS_QUAD_INSTANCE_IND(launch_quad_3x12s7_xi, 3,12,7)
