// Independent<Categorical> (src/codec.rs:366-403) on the fast encoder (ans_mfast.hpp k_menc with
// IndepModel): the instantiations per norm range, renorm screen, lane layout and symbol width.
#include "ans_codecs_indep_impl.hpp"

namespace shuffle_coding {
namespace mfast {

void indep_fast_encode(const IndepFast& f, const EncArgs& a) { indep_enc<false>(f, a); }

}  // namespace mfast
}  // namespace shuffle_coding
