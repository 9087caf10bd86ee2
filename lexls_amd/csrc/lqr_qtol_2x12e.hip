// accuracy-guard instantiation of lqr_qtol_2x12 (the estimate of lqr_qtol_impl.h, EST)
#include "lqr_qtol_impl.h"
LEXLS_QTOL_INSTANCE_EST(launch_qtol_2x12e, 2,12,0,0)
