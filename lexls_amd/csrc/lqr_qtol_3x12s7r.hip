// n = 40, levels of up to 12 rows (per-problem dimensions), x only, tolerance contract: the ragged form
#include "lqr_qtol_impl.h"
LEXLS_QTOL_INSTANCE_RAG(launch_qtol_3x12s7r, 3, 12, 7, 40)
