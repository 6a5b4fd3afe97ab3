// Independent<Categorical> (src/codec.rs:366-403) on the fast decoder (ans_mfast.hpp k_mdec with
// IndepModel): the instantiations per norm range, lean model, lane layout and symbol width.
#include "ans_codecs_indep_impl.hpp"

namespace shuffle_coding {
namespace mfast {

void indep_fast_decode(const IndepFast& f, const DecArgs& a) { indep_dec<false>(f, a); }

}  // namespace mfast
}  // namespace shuffle_coding
