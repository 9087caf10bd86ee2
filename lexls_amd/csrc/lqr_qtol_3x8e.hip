// accuracy-guard instantiation of lqr_qtol_3x8 (the estimate of lqr_qtol_impl.h, EST)
#include "lqr_qtol_impl.h"
LEXLS_QTOL_INSTANCE_EST(launch_qtol_3x8e, 3,8,0,0)
