// Independent<Categorical> resume pops (ans_dev_independent_pop) on the fast decoder (ans_mfast.hpp
// k_mdec<kRes> with IndepModel): the instantiations of ans_codecs_indep_dec.hip again, on the
// message in each slot, in place.
#include "ans_codecs_indep_impl.hpp"

namespace shuffle_coding {
namespace mfast {

void indep_fast_pop(const IndepFast& f, const DecArgs& a) { indep_dec<true>(f, a); }

}  // namespace mfast
}  // namespace shuffle_coding
