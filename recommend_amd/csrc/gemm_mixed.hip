// The whole-tile instantiations of mixed_gemm_kernel (EDGE = false); the edge-tile ones are in gemm.hip, next to
// the dispatch that calls these two functions.
#include "gemm_mixed.h"

namespace ot {

void (*mixed_gemm_whole_for(bool nt, int x, int e, int splt))(GemmArgs) {
  return mixed_gemm_pick<false>(nt, x, e, splt);
}

void (*mixed_gemm_whole_generic(bool nt, int splt))(GemmArgs) { return mixed_gemm_pick_generic<false>(nt, splt); }

}  // namespace ot
