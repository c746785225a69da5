// Batch kernels with a rule per field holding 8 rows in registers (the stepping and the
// period-detecting one); see life_batch_rules.h.  One translation unit per row count
// keeps builds parallel.
#define GOL_BATCH_DEVICE 1
#include "life_batch_rules.h"

namespace gol {
GOL_INSTANTIATE_BATCH_RULES(8)
}  // namespace gol
