// Independent<Categorical> resume pushes (ans_dev_independent_push) on the fast encoder
// (ans_mfast.hpp k_menc<kRes> with IndepModel): the instantiations of ans_codecs_indep_enc.hip
// again, starting from the message in each slot.
#include "ans_codecs_indep_impl.hpp"

namespace shuffle_coding {
namespace mfast {

void indep_fast_push(const IndepFast& f, const EncArgs& a) { indep_enc<true>(f, a); }

}  // namespace mfast
}  // namespace shuffle_coding
