// x only, indirect: the accuracy guard's bit-exact re-solve of the problems lqr_qtol flagged (same arithmetic as lqr_quad_2x12_x)
#include "lqr_quad_impl.h"
LEXLS_QUAD_INSTANCE_IND(launch_quad_2x12_xi, 2,12,0)
