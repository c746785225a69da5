// Batch kernels holding 64 rows in registers (all rule kinds); see life_batch.h.  One
// translation unit per row count keeps builds parallel.
#define GOL_BATCH_DEVICE 1
#include "life_batch.h"

namespace gol {
GOL_INSTANTIATE_BATCH(64)
}  // namespace gol
