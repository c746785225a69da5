// State-recording batch kernels holding 8 rows in registers (all rule kinds, the one
// with a rule per field included); see life_batch_record.h.  One translation unit per row
// count keeps builds parallel.
#define GOL_BATCH_DEVICE 1
#include "life_batch_record.h"

namespace gol {
GOL_INSTANTIATE_BATCH_RECORD(8)
}  // namespace gol
