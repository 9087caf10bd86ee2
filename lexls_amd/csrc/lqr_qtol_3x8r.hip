// 33 .. 48 columns, levels of up to 8 rows (per-problem dimensions), x only, tolerance contract: the ragged form
#include "lqr_qtol_impl.h"
LEXLS_QTOL_INSTANCE_RAG(launch_qtol_3x8r, 3, 8, 0, 0)
