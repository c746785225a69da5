// Period-detecting batch kernels holding 32 rows in registers (all rule kinds); see
// life_batch_until.h.  One translation unit per row count keeps builds parallel.
#define GOL_BATCH_DEVICE 1
#include "life_batch_until.h"

namespace gol {
GOL_INSTANTIATE_BATCH_UNTIL(32)
}  // namespace gol
