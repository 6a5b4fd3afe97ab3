// ans_capi.cpp — host part of the C ABI (include/ans_capi.h sections 1-3).
//
// Message handles, the two-phase scalar op and the single-message IID path run on the
// host because the reference drives them one symbol at a time from sequential callers
// (src/recursive/mod.rs:117-148, src/recursive/prefix_orbit.rs:95-110): there is no
// data parallelism inside one message.  The data-parallel path is section 4
// (ans_pipe.hip for host buffers, ans_kernels.hip for device ones); nothing here is a fallback
// for it.
#include <new>
#include <type_traits>

#include "ans_arer.hpp"
#include "ans_arpu.hpp"
#include "ans_mset.hpp"
#include "ans_polya.hpp"
#include "ans_table.hpp"
#include "ans_joint.hpp"
#include "ans_wl.hpp"

using namespace shuffle_coding;

namespace {

template <class F>
int guarded(F&& f) {
    try {
        f();
        return ANS_OK;
    } catch (const AnsError& e) {
        return e.code;
    } catch (const std::bad_alloc&) {
        return ANS_E_ALLOC;
    } catch (...) {
        return ANS_E_ARG;
    }
}

void check_norm(uint64_t norm) {
    if (norm == 0 || norm > MAX_MIN_HEAD) throw AnsError(ANS_E_NORM_RANGE, "norm out of range");
}

}  // namespace

extern "C" {

const char* ans_status_string(int status) {
    switch (status) {
    case ANS_OK: return "ok";
    case ANS_E_ZERO_MASS: return "zero probability mass for symbol";
    case ANS_E_EXHAUSTED: return "Message exhausted whilst attempting decode.";
    case ANS_E_LEN: return "length mismatch or buffer too small";
    case ANS_E_SYMBOL: return "symbol out of range";
    case ANS_E_NORM_RANGE: return "normaliser / alphabet outside the supported range";
    case ANS_E_DEVICE: return "HIP device error";
    case ANS_E_ALLOC: return "allocation failed";
    case ANS_E_ARG: return "invalid argument";
    case ANS_E_MISMATCH: return "message did not round-trip";
    default: return "unknown status";
    }
}

int ans_abi_version(void) { return 1; }

// ---------------------------------------------------------------- (1) Message
int ans_msg_new(int gen_kind, uint64_t seed, ans_msg** out) {
    if (!out) return ANS_E_ARG;
    *out = nullptr;
    return guarded([&] { *out = new ans_msg{Message::of_kind(gen_kind, seed)}; });
}

void ans_msg_free(ans_msg* m) { delete m; }

int ans_msg_clone(const ans_msg* m, ans_msg** out) {
    if (!m || !out) return ANS_E_ARG;
    *out = nullptr;
    return guarded([&] { *out = new ans_msg{m->m}; });
}

int ans_msg_flatten(const ans_msg* m, uint8_t* out, size_t cap, size_t* len) {
    if (!m || !len) return ANS_E_ARG;
    return guarded([&] {
        const Tail t = m->m.flatten();
        *len = t.elements().size();
        if (!out) return;
        if (cap < *len) throw AnsError(ANS_E_LEN, "flatten buffer too small");
        std::memcpy(out, t.elements().data(), *len);
    });
}

int ans_msg_unflatten(const uint8_t* bytes, size_t len, int gen_kind, uint64_t seed, ans_msg** out) {
    if (!out || (len && !bytes)) return ANS_E_ARG;
    *out = nullptr;
    return guarded([&] {
        std::vector<TailElement> el(bytes, bytes + len);
        *out = new ans_msg{Message::unflatten(Tail(std::move(el), TailGenerator::of_kind(gen_kind, seed)))};
    });
}

int ans_msg_reflatten(const ans_msg* m, ans_msg** out) {
    if (!m || !out) return ANS_E_ARG;
    *out = nullptr;
    return guarded([&] { *out = new ans_msg{Message::unflatten(m->m.flatten())}; });
}

int ans_msg_bits(const ans_msg* m, uint64_t* bits) {
    if (!m || !bits) return ANS_E_ARG;
    return guarded([&] { *bits = m->m.bits(); });
}

int ans_msg_virtual_bits(const ans_msg* m, double* bits) {
    if (!m || !bits) return ANS_E_ARG;
    return guarded([&] { *bits = m->m.virtual_bits(); });
}

int ans_msg_equal(const ans_msg* a, const ans_msg* b, int* equal) {
    if (!a || !b || !equal) return ANS_E_ARG;
    return guarded([&] { *equal = (a->m == b->m) ? 1 : 0; });
}

int ans_msg_state(const ans_msg* m, uint64_t* head, uint64_t* tail_len, uint64_t* num_generated) {
    if (!m) return ANS_E_ARG;
    if (head) *head = m->m.head;
    if (tail_len) *tail_len = m->m.tail.elements().size();
    if (num_generated) *num_generated = m->m.tail.num_generated();
    return ANS_OK;
}

// ---------------------------------------------------------------- (2) two-phase scalar op
int ans_push_begin(ans_msg* m, uint64_t p, uint64_t norm, uint64_t* q, uint64_t* r) {
    if (!m || !q || !r) return ANS_E_ARG;
    return guarded([&] {
        if (p == 0) throw AnsError(ANS_E_ZERO_MASS, "assertion failed: p != 0");  // src/ans.rs:98
        check_norm(norm);
        m->m.renorm(p * (MAX_MIN_HEAD / norm));  // src/ans.rs:100
        *q = m->m.head / p;                      // src/ans.rs:101
        *r = m->m.head % p;                      // src/ans.rs:102
    });
}

int ans_push_end(ans_msg* m, uint64_t norm, uint64_t q, uint64_t cdf) {
    if (!m) return ANS_E_ARG;
    m->m.head = norm * q + cdf;  // src/ans.rs:104
    return ANS_OK;
}

int ans_pop_begin(ans_msg* m, uint64_t norm, uint64_t* q, uint64_t* cf) {
    if (!m || !q || !cf) return ANS_E_ARG;
    return guarded([&] {
        check_norm(norm);
        m->m.renorm(norm * (MAX_MIN_HEAD / norm));  // src/ans.rs:109
        *q = m->m.head / norm;                      // src/ans.rs:110
        *cf = m->m.head % norm;                     // src/ans.rs:111
    });
}

int ans_pop_end(ans_msg* m, uint64_t p, uint64_t q, uint64_t r) {
    if (!m) return ANS_E_ARG;
    m->m.head = p * q + r;  // src/ans.rs:114
    return ANS_OK;
}

int ans_uniform_push(ans_msg* m, uint64_t size, uint64_t x) {
    if (!m) return ANS_E_ARG;
    return guarded([&] {
        const Uniform u(size);
        if (x >= size) throw AnsError(ANS_E_SYMBOL, "symbol out of range");
        u.push(m->m, x);
    });
}

int ans_uniform_pop(ans_msg* m, uint64_t size, uint64_t* x) {
    if (!m || !x) return ANS_E_ARG;
    return guarded([&] {
        const Uniform u(size);
        *x = u.pop(m->m);
    });
}

// ---------------------------------------------------------------- (3) tables
int ans_table_create(const uint64_t* masses, uint32_t nsym, ans_table** out) {
    if (!out || (nsym && !masses)) return ANS_E_ARG;
    *out = nullptr;
    return guarded([&] {
        uint64_t acc = 0;
        for (uint32_t s = 0; s < nsym; ++s) {
            if (masses[s] > MAX_MIN_HEAD - acc) throw AnsError(ANS_E_NORM_RANGE, "sum of masses overflows");
            acc += masses[s];
        }
        *out = new ans_table{Categorical(std::vector<uint64_t>(masses, masses + nsym))};
    });
}

int ans_table_create_bernoulli(uint64_t mass, uint64_t norm, ans_table** out) {
    if (!out) return ANS_E_ARG;
    *out = nullptr;
    return guarded([&] {
        const Bernoulli b(mass, norm);
        *out = new ans_table{b.categorical};
    });
}

void ans_table_free(ans_table* t) { delete t; }

int ans_table_info(const ans_table* t, uint32_t* nsym, uint64_t* norm) {
    if (!t) return ANS_E_ARG;
    if (nsym) *nsym = static_cast<uint32_t>(t->cat.masses.size());
    if (norm) *norm = t->cat.norm();
    return ANS_OK;
}

int ans_cat_push(ans_msg* m, const ans_table* t, uint64_t x) {
    if (!m || !t) return ANS_E_ARG;
    return guarded([&] { t->cat.push(m->m, x); });
}

int ans_cat_pop(ans_msg* m, const ans_table* t, uint64_t* x) {
    if (!m || !t || !x) return ANS_E_ARG;
    return guarded([&] { *x = t->cat.pop(m->m); });
}

int ans_push_iid(ans_msg* m, const ans_table* t, const uint32_t* syms, size_t n) {
    if (!m || !t || (n && !syms)) return ANS_E_ARG;
    return guarded([&] {
        for (size_t k = n; k-- > 0;) t->cat.push(m->m, static_cast<uint64_t>(syms[k]));  // src/codec.rs:417
    });
}

int ans_pop_iid(ans_msg* m, const ans_table* t, uint32_t* out, size_t n) {
    if (!m || !t || (n && !out)) return ANS_E_ARG;
    return guarded([&] {
        for (size_t k = 0; k < n; ++k) out[k] = static_cast<uint32_t>(t->cat.pop(m->m));  // src/codec.rs:423
    });
}

// ---- recursive multiset shuffle coding on one message (ans_mset.hpp): ShuffleCodec<
// IIDVecSliceCodecs<Categorical>, VecOrbitCodecs>, src/recursive/mod.rs:117-148
uint64_t ans_orbit_id(uint64_t x) { return mset::orbit_id(x); }

namespace {
struct VecAcc {  // the counts' nodes in a vector
    uint32_t* p;
    uint32_t load(uint32_t i) const { return p[i]; }
    void store(uint32_t i, uint32_t v) { p[i] = v; }
};
// the table's rank tables (built once per table; ANS_E_ARG for an alphabet the codec does not take)
void need_ranks(const ans_table* t) {
    const size_t nsym = t->cat.masses.size();
    if (nsym == 0 || nsym > mset::kMaxSymbols) throw AnsError(ANS_E_ARG, "multiset alphabet outside 1..65536 symbols");
    std::call_once(t->ranks_once,
                   [&] { t->ranks_ok = mset::build_ranks(static_cast<uint32_t>(nsym), t->rank, t->sym_of_rank); });
    if (!t->ranks_ok) throw AnsError(ANS_E_ARG, "two symbols share an orbit id");
}
}  // namespace

int ans_mset_push(ans_msg* m, const ans_table* t, const uint32_t* syms, size_t n) {
    if (!m || !t || (n && !syms)) return ANS_E_ARG;
    return guarded([&] {
        need_ranks(t);
        if (n > 0xFFFFFFFFull) throw AnsError(ANS_E_ARG, "multiset of 2^32 or more values");
        const Categorical& cat = t->cat;
        const uint32_t nsym = static_cast<uint32_t>(cat.masses.size());
        std::vector<uint32_t> nodes(nsym, 0);
        mset::Counts<VecAcc> cnt{VecAcc{nodes.data()}, nsym};
        for (size_t k = 0; k < n; ++k) {
            if (cat.pmf(syms[k]) == 0) throw AnsError(ANS_E_ZERO_MASS, "assertion failed: pmf(x) != 0");
            cnt.tally(t->rank[syms[k]]);
        }
        cnt.build();
        Message& msg = m->m;
        for (uint64_t L = n; L > 0; --L) {
            // pop a rank under the orbit distribution of the L values left (src/ans.rs:107-116)
            msg.renorm(L * (MAX_MIN_HEAD / L));
            const uint64_t q = msg.head / L, cf = msg.head % L;
            const mset::Found f = cnt.find(cf);
            msg.head = f.count * q + (cf - f.cum);
            cnt.add(f.rank, -1);
            cat.push(msg, static_cast<uint64_t>(t->sym_of_rank[f.rank]));  // ... and push its symbol
        }
    });
}

int ans_mset_pop(ans_msg* m, const ans_table* t, uint32_t* out, size_t n) {
    if (!m || !t || (n && !out)) return ANS_E_ARG;
    return guarded([&] {
        need_ranks(t);
        if (n > 0xFFFFFFFFull) throw AnsError(ANS_E_ARG, "multiset of 2^32 or more values");
        const Categorical& cat = t->cat;
        const uint32_t nsym = static_cast<uint32_t>(cat.masses.size());
        std::vector<uint32_t> nodes(nsym, 0);
        mset::Counts<VecAcc> cnt{VecAcc{nodes.data()}, nsym};
        Message& msg = m->m;
        for (uint64_t k = 0; k < n; ++k) {
            const uint64_t s = cat.pop(msg);
            out[k] = static_cast<uint32_t>(s);
            const uint32_t r = t->rank[s];
            cnt.add(r, 1);
            // push the rank under the orbit distribution of the k + 1 values so far (src/ans.rs:96-105)
            const uint64_t p = cnt.count(r), c = cnt.prefix(r), norm = k + 1;
            msg.renorm(p * (MAX_MIN_HEAD / norm));
            msg.head = norm * (msg.head / p) + c + msg.head % p;
        }
    });
}

// ---- the Pólya urn edge-index codec on one message (ans_polya.hpp): multiset_shuffle_codec(
// PolyaUrnEdgeIndicesCodec<Undirected>), src/graph_codec.rs:210-375
extern "C++" {
namespace {
struct VecWs {  // the state's arrays, one after the other in a vector
    uint32_t* p;
    VecAcc at(uint64_t o) const { return VecAcc{p + o}; }
};
struct HostMsg {  // a Message as polya::Coder takes it
    Message& msg;
    uint64_t& head;
    bool renorm(uint64_t min_head) {
        try {
            msg.renorm(min_head);
            return true;
        } catch (const AnsError&) {  // the Empty generator, src/ans.rs:144
            return false;
        }
    }
};
template <class F>
int polya_host(ans_msg* m, uint32_t num_nodes, size_t num_edges, F&& f) {
    return guarded([&] {
        if (num_edges > polya::kMaxEdges) throw AnsError(ANS_E_ARG, "2^31 or more edges");
        std::vector<uint32_t> ws(polya::ws_entries(num_nodes, num_edges));
        auto st = polya::State<VecAcc>::make(VecWs{ws.data()}, num_nodes, num_edges);
        HostMsg hm{m->m, m->m.head};
        polya::Coder<HostMsg> c{hm, ANS_OK};
        if (const int rc = f(c, st)) throw AnsError(rc, ans_status_string(rc));
    });
}
}  // namespace
}  // extern "C++" (templates)

int ans_polya_push(ans_msg* m, uint32_t num_nodes, int loops, int redraws, const uint32_t* edges, size_t num_edges) {
    if (!m || (num_edges && !edges)) return ANS_E_ARG;
    return polya_host(m, num_nodes, num_edges, [&](auto& c, auto& st) {
        return polya::push_graph(c, st, num_nodes, loops != 0, redraws != 0, edges, static_cast<uint32_t>(num_edges));
    });
}

int ans_polya_pop(ans_msg* m, uint32_t num_nodes, int loops, int redraws, uint32_t* edges, size_t num_edges) {
    if (!m || (num_edges && !edges)) return ANS_E_ARG;
    return polya_host(m, num_nodes, num_edges, [&](auto& c, auto& st) {
        return polya::pop_graph(c, st, num_nodes, loops != 0, redraws != 0, edges, static_cast<uint32_t>(num_edges));
    });
}

// ---- recursive shuffle coding of a graph on one message (ans_rgraph.hpp): the autoregressive
// Erdős–Rényi (ans_arer.hpp) and Pólya urn (ans_arpu.hpp) slices, as a labelled graph or under the
// orbits of wl_iter = 0 as counts per class (Autoregressive(..) and ShuffleCodec<.., WLOrbitCodecs>,
// src/recursive/mod.rs:117-216, src/recursive/graph/slice.rs, incomplete.rs:189-236), or with
// Weisfeiler-Lehman orbits at wl_iter <= ANS_WL_MAX_ITER (ans_wl.hpp: incomplete.rs:45-57, 87-151)
extern "C++" {
namespace {
struct SizedWs {  // the states name each array's length; a vector needs only its start
    uint32_t* p;
    VecAcc at(uint64_t o, uint64_t) const { return VecAcc{p + o}; }
};
// an orbit stage's setting: checked, then what the state's make takes after the bounds
struct CountSetting {
    int orbits;
    std::vector<uint32_t> rank;
    void check(uint32_t num_nodes) {
        if (orbits != ANS_ORBITS_NONE && orbits != ANS_ORBITS_ONE_CLASS && orbits != ANS_ORBITS_DEGREE)
            throw AnsError(ANS_E_ARG, "orbits outside NONE, ONE_CLASS, DEGREE");
        if (num_nodes > 0x7FFFFFFFu) throw AnsError(ANS_E_ARG, "2^31 or more nodes");
        if (orbits == ANS_ORBITS_DEGREE && !arer::build_degree_ranks(num_nodes, rank))
            throw AnsError(ANS_E_ARG, "two degrees share a class id");
    }
    template <class St>
    St make(const SizedWs& ws, uint32_t num_nodes, uint64_t max_edges) const {
        return St::make(ws, num_nodes, max_edges, orbits, static_cast<const uint32_t*>(rank.data()), num_nodes + 1);
    }
};
struct WlSetting {
    int wl_iter, half_iter;
    void check(uint32_t num_nodes) const {
        if (wl_iter < 0 || wl_iter > ANS_WL_MAX_ITER) throw AnsError(ANS_E_ARG, "wl_iter outside 0 .. ANS_WL_MAX_ITER");
        if (!wl::nodes_ok(num_nodes, wl_iter)) throw AnsError(ANS_E_ARG, "2^31 or more nodes, or 2^32 or more id words");
    }
    template <class St>
    St make(const SizedWs& ws, uint32_t num_nodes, uint64_t max_edges) const {
        return St::make(ws, num_nodes, max_edges, static_cast<uint32_t>(wl_iter), half_iter != 0);
    }
};
void set_bern(arer::ErSlices<VecAcc>& s, const ans_table* bern) {
    s.bern = arer::bern_of(bern->cat.masses[0], bern->cat.masses[1]);
}
void set_bern(arpu::PuSlices<VecAcc>&, const ans_table*) {}

using CountRank = const uint32_t*;
// St over a vector of `entries`, bounded by num_nodes and max_edges; run(coder, state) is the codec.
// bern: the table of the Erdős–Rényi slices, null for the Pólya urn's.
template <class St, class Setting, class Run>
int graph_host(ans_msg* m, const ans_table* bern, Setting setting, uint64_t entries, uint32_t num_nodes, uint64_t max_edges,
               Run&& run) {
    return guarded([&] {
        if (bern && bern->cat.masses.size() != 2) throw AnsError(ANS_E_ARG, "the indicator table needs exactly two symbols");
        setting.check(num_nodes);
        std::vector<uint32_t> ws(entries);
        St st = setting.template make<St>(SizedWs{ws.data()}, num_nodes, max_edges);
        set_bern(st, bern);
        HostMsg hm{m->m, m->m.head};
        polya::Coder<HostMsg> c{hm, ANS_OK};
        if (const int rc = run(c, st)) throw AnsError(rc, ans_status_string(rc));
    });
}
template <class St, class Setting>
int graph_push(ans_msg* m, const ans_table* bern, Setting setting, uint64_t entries, uint32_t num_nodes, int loops,
               const uint32_t* edges, size_t num_edges, uint32_t* perm) {
    return graph_host<St>(m, bern, std::move(setting), entries, num_nodes, num_edges, [&](auto& c, St& st) {
        return rgraph::push_graph(c, st, num_nodes, loops != 0, edges, static_cast<uint32_t>(num_edges), perm);
    });
}
// room: the pairs the state is bounded by; at most cap of them come out
template <class St, class Setting>
int graph_pop(ans_msg* m, const ans_table* bern, Setting setting, uint64_t entries, uint32_t num_nodes, uint64_t room,
              int loops, uint32_t* edges, uint64_t cap, size_t* num_edges) {
    return graph_host<St>(m, bern, std::move(setting), entries, num_nodes, room, [&](auto& c, St& st) {
        uint64_t count = 0;
        const int rc = rgraph::pop_graph(c, st, num_nodes, loops != 0, edges, cap, &count);
        *num_edges = static_cast<size_t>(count);
        return rc;
    });
}
// (no graph holds more pairs than its alphabet: a larger cap sizes nothing)
uint64_t pop_room(uint32_t num_nodes, size_t cap) {
    return std::min<uint64_t>({cap, uint64_t(num_nodes) * (num_nodes + 1) / 2, rgraph::kMaxEdges});
}
}  // namespace
}  // extern "C++" (templates)

int ans_ar_er_push(ans_msg* m, const ans_table* bern, uint32_t num_nodes, int loops, int orbits, const uint32_t* edges,
                   size_t num_edges, uint32_t* perm) {
    if (!m || !bern || (num_edges && !edges) || num_edges > arer::kMaxEdges) return ANS_E_ARG;
    return graph_push<arer::PushState<VecAcc, CountRank>>(m, bern, CountSetting{orbits, {}},
                                                          arer::push_entries(num_nodes, num_edges), num_nodes, loops, edges,
                                                          num_edges, perm);
}

int ans_ar_er_pop(ans_msg* m, const ans_table* bern, uint32_t num_nodes, int loops, int orbits, uint32_t* edges,
                  size_t cap, size_t* num_edges) {
    if (!m || !bern || !num_edges || (cap && !edges)) return ANS_E_ARG;
    *num_edges = 0;
    return graph_pop<arer::PopState<VecAcc, CountRank>>(m, bern, CountSetting{orbits, {}}, arer::pop_entries(num_nodes),
                                                        num_nodes, 0, loops, edges, cap, num_edges);
}

int ans_ar_polya_push(ans_msg* m, uint32_t num_nodes, int loops, int orbits, const uint32_t* edges, size_t num_edges,
                      uint32_t* perm) {
    if (!m || (num_edges && !edges) || num_edges > arpu::kMaxEdges) return ANS_E_ARG;
    return graph_push<arpu::PushState<VecAcc, CountRank>>(m, nullptr, CountSetting{orbits, {}},
                                                          arpu::push_entries(num_nodes, num_edges), num_nodes, loops, edges,
                                                          num_edges, perm);
}

int ans_ar_polya_pop(ans_msg* m, uint32_t num_nodes, int loops, int orbits, uint32_t* edges, size_t cap,
                     size_t* num_edges) {
    if (!m || !num_edges || (cap && !edges)) return ANS_E_ARG;
    *num_edges = 0;
    return graph_pop<arpu::PopState<VecAcc, CountRank>>(m, nullptr, CountSetting{orbits, {}}, arpu::pop_entries(num_nodes),
                                                        num_nodes, 0, loops, edges, cap, num_edges);
}

int ans_ar_er_wl_push(ans_msg* m, const ans_table* bern, uint32_t num_nodes, int loops, int wl_iter, int half_iter,
                      const uint32_t* edges, size_t num_edges, uint32_t* perm) {
    if (!m || !bern || (num_edges && !edges) || num_edges > arer::kMaxEdges) return ANS_E_ARG;
    return graph_push<wl::ErPush<VecAcc>>(m, bern, WlSetting{wl_iter, half_iter},
                                          wl::er_push_entries(num_nodes, num_edges, wl_iter), num_nodes, loops, edges,
                                          num_edges, perm);
}

int ans_ar_er_wl_pop(ans_msg* m, const ans_table* bern, uint32_t num_nodes, int loops, int wl_iter, int half_iter,
                     uint32_t* edges, size_t cap, size_t* num_edges) {
    if (!m || !bern || !num_edges || (cap && !edges)) return ANS_E_ARG;
    *num_edges = 0;
    const uint64_t room = pop_room(num_nodes, cap);
    return graph_pop<wl::ErPop<VecAcc>>(m, bern, WlSetting{wl_iter, half_iter}, wl::er_pop_entries(num_nodes, room, wl_iter),
                                        num_nodes, room, loops, edges, room, num_edges);
}

int ans_ar_polya_wl_push(ans_msg* m, uint32_t num_nodes, int loops, int wl_iter, int half_iter, const uint32_t* edges,
                         size_t num_edges, uint32_t* perm) {
    if (!m || (num_edges && !edges) || num_edges > arpu::kMaxEdges) return ANS_E_ARG;
    return graph_push<wl::PuPush<VecAcc>>(m, nullptr, WlSetting{wl_iter, half_iter},
                                          wl::pu_push_entries(num_nodes, num_edges, wl_iter), num_nodes, loops, edges,
                                          num_edges, perm);
}

int ans_ar_polya_wl_pop(ans_msg* m, uint32_t num_nodes, int loops, int wl_iter, int half_iter, uint32_t* edges,
                        size_t cap, size_t* num_edges) {
    if (!m || !num_edges || (cap && !edges)) return ANS_E_ARG;
    *num_edges = 0;
    const uint64_t room = pop_room(num_nodes, cap);
    return graph_pop<wl::PuPop<VecAcc>>(m, nullptr, WlSetting{wl_iter, half_iter}, wl::pu_pop_entries(num_nodes, room, wl_iter),
                                        num_nodes, room, loops, edges, room, num_edges);
}

// ---- joint shuffle coding of a graph on one message (ans_joint.hpp): ShuffleCodec<JointSliceCodecs<C>,
// WLOrbitCodecs<JointPrefix<Graph>>> (src/recursive/joint.rs, incomplete.rs:154-187) with C the dense
// Erdős–Rényi indicator or the ordered Pólya urn.  A failed call puts the message back as it found it.
extern "C++" {
namespace {
void set_bern(joint::ErPush<VecAcc>& s, const ans_table* bern) { s.bern = arer::bern_of(bern->cat.masses[0], bern->cat.masses[1]); }
void set_bern(joint::ErPop<VecAcc>& s, const ans_table* bern) { s.bern = arer::bern_of(bern->cat.masses[0], bern->cat.masses[1]); }
void set_bern(joint::PuPush<VecAcc>&, const ans_table*) {}
void set_bern(joint::PuPop<VecAcc>&, const ans_table*) {}
template <class St, class Run>
int joint_host(ans_msg* m, const ans_table* bern, int wl_iter, int half_iter, uint64_t entries, uint32_t num_nodes,
               uint64_t max_edges, Run&& run) {
    const Message before = m->m;
    const int rc = graph_host<St>(m, bern, WlSetting{wl_iter, half_iter}, entries, num_nodes, max_edges, run);
    if (rc) m->m = before;
    return rc;
}
uint32_t wl_or_0(int wl_iter) { return wl_iter >= 0 && wl_iter <= ANS_WL_MAX_ITER ? wl_iter : 0; }  // (the setting's check refuses the rest)
}  // namespace
}  // extern "C++" (templates)

int ans_joint_er_wl_push(ans_msg* m, const ans_table* bern, uint32_t num_nodes, int loops, int wl_iter, int half_iter,
                         const uint32_t* edges, size_t num_edges, uint32_t* perm) {
    if (!m || !bern || (num_edges && !edges) || num_edges > arer::kMaxEdges) return ANS_E_ARG;
    using St = joint::ErPush<VecAcc>;
    return joint_host<St>(m, bern, wl_iter, half_iter, joint::er_push_entries(num_nodes, num_edges, wl_or_0(wl_iter)), num_nodes,
                          num_edges, [&](auto& c, St& st) {
                              return joint::push_joint(c, st, num_nodes, loops != 0, edges, static_cast<uint32_t>(num_edges), perm);
                          });
}

int ans_joint_er_wl_pop(ans_msg* m, const ans_table* bern, uint32_t num_nodes, int loops, int wl_iter, int half_iter,
                        uint32_t* edges, size_t cap, size_t* num_edges) {
    if (!m || !bern || !num_edges || (cap && !edges)) return ANS_E_ARG;
    *num_edges = 0;
    using St = joint::ErPop<VecAcc>;
    const uint64_t room = pop_room(num_nodes, cap);
    return joint_host<St>(m, bern, wl_iter, half_iter, joint::er_pop_entries(num_nodes, room, wl_or_0(wl_iter)), num_nodes, room,
                          [&](auto& c, St& st) {
                              uint64_t count = 0;
                              const int rc = joint::pop_joint(c, st, num_nodes, loops != 0, edges, room, &count);
                              *num_edges = static_cast<size_t>(count);
                              return rc;
                          });
}

int ans_joint_polya_wl_push(ans_msg* m, uint32_t num_nodes, int loops, int redraws, int wl_iter, int half_iter,
                            const uint32_t* edges, size_t num_edges, uint32_t* perm) {
    if (!m || (num_edges && !edges) || num_edges > polya::kMaxEdges) return ANS_E_ARG;
    using St = joint::PuPush<VecAcc>;
    return joint_host<St>(m, nullptr, wl_iter, half_iter, joint::pu_push_entries(num_nodes, num_edges, wl_or_0(wl_iter)),
                          num_nodes, num_edges, [&](auto& c, St& st) {
                              st.redraws = redraws != 0;
                              return joint::push_joint(c, st, num_nodes, loops != 0, edges, static_cast<uint32_t>(num_edges), perm);
                          });
}

int ans_joint_polya_wl_pop(ans_msg* m, uint32_t num_nodes, int loops, int redraws, int wl_iter, int half_iter,
                           uint32_t* edges, size_t num_edges) {
    if (!m || (num_edges && !edges) || num_edges > polya::kMaxEdges) return ANS_E_ARG;
    using St = joint::PuPop<VecAcc>;
    return joint_host<St>(m, nullptr, wl_iter, half_iter, joint::pu_pop_entries(num_nodes, num_edges, wl_or_0(wl_iter)), num_nodes,
                          num_edges, [&](auto& c, St& st) {
                              st.redraws = redraws != 0;
                              uint64_t count = 0;
                              return joint::pop_joint(c, st, num_nodes, loops != 0, edges, num_edges, &count);
                          });
}

// ---- ... of a graph with node and edge labels (Graph<N, E, Undirected>, N and E each usize or ();
// src/recursive/graph/mod.rs:53-104, incomplete.rs:45-57, 97-151, 193-210): a NULL table is
// EmptyCodec, the label absent
extern "C++" {
namespace {
// a table as the recursion's Categorical step takes it; cum keeps the cdf with the norm behind it
rgraph::Cat host_cat(const ans_table* t, std::vector<uint64_t>& cum) {
    if (!t) return rgraph::Cat{};
    check_norm(t->cat.norm());
    if (t->cat.masses.size() > 0xFFFFFFFFull) throw AnsError(ANS_E_NORM_RANGE, "2^32 or more label symbols");
    cum = t->cat.cummasses;
    cum.push_back(t->cat.norm());
    return rgraph::Cat{cum.data(), nullptr, t->cat.norm(), static_cast<uint32_t>(t->cat.masses.size()), 0};
}
template <class F>
int with_labels(bool node, bool edge, F&& f) {
    if (node) return edge ? f(rgraph::Labels<true, true>{}) : f(rgraph::Labels<true, false>{});
    return edge ? f(rgraph::Labels<false, true>{}) : f(rgraph::Labels<false, false, true>{});
}
// kEr: the Erdős–Rényi slices under bern, else the Pólya urn's
template <bool kEr>
int labelled_push(ans_msg* m, const ans_table* bern, uint32_t num_nodes, int loops, int wl_iter, int half_iter,
                  const uint32_t* edges, size_t num_edges, uint32_t* perm, const ans_table* node, const ans_table* edge,
                  const uint32_t* node_labels, const uint32_t* edge_labels) {
    if (!m || (kEr && !bern) || (num_edges && !edges) || num_edges > rgraph::kMaxEdges || !node != !node_labels ||
        !edge != !edge_labels)
        return ANS_E_ARG;
    return with_labels(node, edge, [&](auto labels) {
        using L = decltype(labels);
        using St = std::conditional_t<kEr, wl::ErPush<VecAcc, L>, wl::PuPush<VecAcc, L>>;
        const uint32_t w = wl_iter >= 0 && wl_iter <= ANS_WL_MAX_ITER ? wl_iter : 0;  // (the setting's check refuses the rest)
        const uint64_t entries = kEr ? wl::er_push_entries(num_nodes, num_edges, w, L::edge)
                                     : wl::pu_push_entries(num_nodes, num_edges, w, L::edge);
        std::vector<uint64_t> node_cum, edge_cum;
        return graph_host<St>(m, bern, WlSetting{wl_iter, half_iter}, entries, num_nodes, num_edges, [&](auto& c, St& st) {
            if constexpr (L::any) {
                st.lab.node = host_cat(node, node_cum);
                st.lab.edge = host_cat(edge, edge_cum);
                st.lab.nl = node_labels;
                st.lab.el = edge_labels;
            }
            return rgraph::push_graph(c, st, num_nodes, loops != 0, edges, static_cast<uint32_t>(num_edges), perm);
        });
    });
}
template <bool kEr>
int labelled_pop(ans_msg* m, const ans_table* bern, uint32_t num_nodes, int loops, int wl_iter, int half_iter,
                 uint32_t* edges, size_t cap, size_t* num_edges, const ans_table* node, const ans_table* edge,
                 uint32_t* node_labels, uint32_t* edge_labels) {
    if (!m || (kEr && !bern) || !num_edges || (cap && !edges) || !node != !node_labels || !edge != !edge_labels)
        return ANS_E_ARG;
    *num_edges = 0;
    const uint64_t room = pop_room(num_nodes, cap);
    return with_labels(node, edge, [&](auto labels) {
        using L = decltype(labels);
        using St = std::conditional_t<kEr, wl::ErPop<VecAcc, L>, wl::PuPop<VecAcc, L>>;
        const uint32_t w = wl_iter >= 0 && wl_iter <= ANS_WL_MAX_ITER ? wl_iter : 0;
        const uint64_t entries = kEr ? wl::er_pop_entries(num_nodes, room, w, L::edge) : wl::pu_pop_entries(num_nodes, room, w, L::edge);
        std::vector<uint64_t> node_cum, edge_cum;
        return graph_host<St>(m, bern, WlSetting{wl_iter, half_iter}, entries, num_nodes, room, [&](auto& c, St& st) {
            st.lab = rgraph::PopLabels{host_cat(node, node_cum), host_cat(edge, edge_cum), node_labels, edge_labels};
            uint64_t count = 0;
            const int rc = rgraph::pop_graph(c, st, num_nodes, loops != 0, edges, room, &count);
            *num_edges = static_cast<size_t>(count);
            return rc;
        });
    });
}
}  // namespace
}  // extern "C++" (templates)

int ans_ar_er_wl_labelled_push(ans_msg* m, const ans_table* bern, uint32_t num_nodes, int loops, int wl_iter,
                               int half_iter, const uint32_t* edges, size_t num_edges, uint32_t* perm,
                               const ans_table* node, const ans_table* edge, const uint32_t* node_labels,
                               const uint32_t* edge_labels) {
    return labelled_push<true>(m, bern, num_nodes, loops, wl_iter, half_iter, edges, num_edges, perm, node, edge,
                               node_labels, edge_labels);
}

int ans_ar_er_wl_labelled_pop(ans_msg* m, const ans_table* bern, uint32_t num_nodes, int loops, int wl_iter,
                              int half_iter, uint32_t* edges, size_t cap, size_t* num_edges, const ans_table* node,
                              const ans_table* edge, uint32_t* node_labels, uint32_t* edge_labels) {
    return labelled_pop<true>(m, bern, num_nodes, loops, wl_iter, half_iter, edges, cap, num_edges, node, edge,
                              node_labels, edge_labels);
}

int ans_ar_polya_wl_labelled_push(ans_msg* m, uint32_t num_nodes, int loops, int wl_iter, int half_iter,
                                  const uint32_t* edges, size_t num_edges, uint32_t* perm, const ans_table* node,
                                  const ans_table* edge, const uint32_t* node_labels, const uint32_t* edge_labels) {
    return labelled_push<false>(m, nullptr, num_nodes, loops, wl_iter, half_iter, edges, num_edges, perm, node, edge,
                                node_labels, edge_labels);
}

int ans_ar_polya_wl_labelled_pop(ans_msg* m, uint32_t num_nodes, int loops, int wl_iter, int half_iter, uint32_t* edges,
                                 size_t cap, size_t* num_edges, const ans_table* node, const ans_table* edge,
                                 uint32_t* node_labels, uint32_t* edge_labels) {
    return labelled_pop<false>(m, nullptr, num_nodes, loops, wl_iter, half_iter, edges, cap, num_edges, node, edge,
                               node_labels, edge_labels);
}

}  // extern "C"
