/*
 * ans_capi.h — C ABI of the MI355X-native rANS coder (libshufflecoding_amd.so).
 *
 * This is the drop-in boundary for the reference's ANS hot path
 * (entropy-coding/shuffle-coding @ 2024_08_07).  Plain pointers and sizes only; no
 * exceptions cross it; caller-owned buffers; no pointer is retained after a call
 * returns (handles excepted).  Every entry point names the reference interface it
 * replaces.  A Rust caller binds it with an `extern "C"` block.
 *
 * Threading: a Message handle is single-threaded (the reference's `&mut Message`);
 * tables are immutable after creation and may be shared; GPU handles are per device,
 * one HIP stream each, and must not be used from two threads at once.  A GPU table or
 * table set may be freed before or after its context (the free touches only the table,
 * e.g. from a garbage collector that finalizes both in any order); every other call on it
 * needs its context alive.
 */
#ifndef ANS_CAPI_H
#define ANS_CAPI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes (the reference panics; we return these instead) ---- */
#define ANS_OK 0
#define ANS_E_ZERO_MASS 1   /* src/ans.rs:98     assert_ne!(p, 0)                        */
#define ANS_E_EXHAUSTED 2   /* src/ans.rs:144    "Message exhausted whilst attempting decode." */
#define ANS_E_LEN 3         /* src/codec.rs:416  IID length assert / output buffer too small  */
#define ANS_E_SYMBOL 4      /* src/codec.rs:63   symbol index out of range                */
#define ANS_E_NORM_RANGE 5  /* src/codec.rs:35   size/norm outside what the coder supports */
#define ANS_E_DEVICE 6      /* HIP runtime error or no GPU                                */
#define ANS_E_ALLOC 7       /* host or device allocation failed                           */
#define ANS_E_ARG 8         /* invalid argument (NULL handle, bad width, ...)             */
#define ANS_E_MISMATCH 9    /* a reference property check failed (src/ans.rs:52-57)       */

/* ---- tail generators: src/ans.rs:131-136 TailGenerator ---- */
#define ANS_GEN_ZEROS 0  /* Message::zeros()  src/ans.rs:292 */
#define ANS_GEN_EMPTY 1  /* Message::empty()  src/ans.rs:297 */
#define ANS_GEN_RANDOM 2 /* Message::random() src/ans.rs:285 (PCG bytes parity-unpinned) */

const char *ans_status_string(int status);
int ans_abi_version(void); /* bumps on any incompatible change */

/* ======================================================================
 * (1) Message handle — replaces `pub struct Message { head, tail }`
 *     (src/ans.rs:225-310).
 * ====================================================================== */
typedef struct ans_msg ans_msg;

/* Message::zeros()/empty()/random(seed)  src/ans.rs:285-299 */
int ans_msg_new(int gen_kind, uint64_t seed, ans_msg **out);
void ans_msg_free(ans_msg *m);
/* Clone  (#[derive(Clone)] src/ans.rs:225) */
int ans_msg_clone(const ans_msg *m, ans_msg **out);
/* m.clone().flatten().elements  src/ans.rs:255-260.  *len receives the byte count;
 * with out == NULL or cap < *len nothing is copied (size query / ANS_E_LEN). */
int ans_msg_flatten(const ans_msg *m, uint8_t *out, size_t cap, size_t *len);
/* Message::unflatten(Tail::new(bytes, generator))  src/ans.rs:262-264 */
int ans_msg_unflatten(const uint8_t *bytes, size_t len, int gen_kind, uint64_t seed, ans_msg **out);
/* Message::unflatten(m.clone().flatten()) keeping the Tail's generator state and
 * num_generated, as the reference's round-trip check does (src/ans.rs:57) */
int ans_msg_reflatten(const ans_msg *m, ans_msg **out);
/* Message::bits / virtual_bits  src/ans.rs:267-283 */
int ans_msg_bits(const ans_msg *m, uint64_t *bits);
int ans_msg_virtual_bits(const ans_msg *m, double *bits);
/* PartialEq for Message (canonicalising)  src/ans.rs:302-310 */
int ans_msg_equal(const ans_msg *a, const ans_msg *b, int *equal);
/* field access: m.head, m.tail.elements.len(), m.tail.num_generated */
int ans_msg_state(const ans_msg *m, uint64_t *head, uint64_t *tail_len, uint64_t *num_generated);

/* ======================================================================
 * (2) Two-phase scalar op — replaces the blanket `impl<D: Distribution> Codec for D`
 *     (src/ans.rs:93-121) for ANY Distribution, including ones whose cdf depends on i
 *     (e.g. PlainOrbitCodec, src/recursive/plain_orbit.rs:33-49).
 *       push: ans_push_begin(m, pmf(x), norm, &q, &r); c = cdf(x, r); ans_push_end(m, norm, q, c)
 *       pop:  ans_pop_begin(m, norm, &q, &cf); (x, r) = icdf(cf); ans_pop_end(m, pmf(x), q, r)
 * ====================================================================== */
int ans_push_begin(ans_msg *m, uint64_t p, uint64_t norm, uint64_t *q, uint64_t *r); /* ans.rs:97-102 */
int ans_push_end(ans_msg *m, uint64_t norm, uint64_t q, uint64_t cdf);               /* ans.rs:103-104 */
int ans_pop_begin(ans_msg *m, uint64_t norm, uint64_t *q, uint64_t *cf);             /* ans.rs:108-111 */
int ans_pop_end(ans_msg *m, uint64_t p, uint64_t q, uint64_t r);                     /* ans.rs:112-114 */
/* Uniform::push/pop  src/codec.rs:18-31 (size <= MAX_SIZE = 2^46, src/ans.rs:22) */
int ans_uniform_push(ans_msg *m, uint64_t size, uint64_t x);
int ans_uniform_pop(ans_msg *m, uint64_t size, uint64_t *x);

/* ======================================================================
 * (3) Static tables — replaces `Categorical` / `Bernoulli` (src/codec.rs:51-129) and
 *     `IID<Categorical>` on ONE message (src/codec.rs:405-443), on the host.
 * ====================================================================== */
typedef struct ans_table ans_table;

/* Categorical::new(masses)  src/codec.rs:72-80 */
int ans_table_create(const uint64_t *masses, uint32_t nsym, ans_table **out);
/* Bernoulli::new(mass, norm) = Categorical[norm-mass, mass]  src/codec.rs:125-128 */
int ans_table_create_bernoulli(uint64_t mass, uint64_t norm, ans_table **out);
void ans_table_free(ans_table *t);
int ans_table_info(const ans_table *t, uint32_t *nsym, uint64_t *norm);
/* Categorical as a Codec (blanket impl)  src/ans.rs:96-116 */
int ans_cat_push(ans_msg *m, const ans_table *t, uint64_t x);
int ans_cat_pop(ans_msg *m, const ans_table *t, uint64_t *x);
/* IID::push (reverse order) / IID::pop (forward)  src/codec.rs:415-424 */
int ans_push_iid(ans_msg *m, const ans_table *t, const uint32_t *syms, size_t n);
int ans_pop_iid(ans_msg *m, const ans_table *t, uint32_t *out, size_t n);
/* Recursive multiset shuffle coding of n values of the table's alphabet as ONE multiset:
 * ShuffleCodec<IIDVecSliceCodecs<Categorical>, VecOrbitCodecs>  src/recursive/mod.rs:117-148,
 * src/recursive/multiset.rs:13-91,139-141 (the harness's iid_multiset_shuffle_codec).
 *   push: the order of syms does not matter.  For L = n .. 1: a value's orbit is POPPED under the
 *         orbit distribution of the L values left (a MutCategorical keyed by orbit id,
 *         src/codec.rs:145-181: norm L, pmf = how many of them are that value, orbits in ascending
 *         id order), the value leaves the multiset and is pushed under the table.
 *   pop:  for k = 0 .. n-1: a value is popped under the table, joins the multiset, and its orbit is
 *         PUSHED under the orbit distribution of the k + 1 values so far.  out receives the values
 *         in pop order (the reference wraps them as Unordered); that order is deterministic.
 * ans_orbit_id(x) is the orbit id of value x: hash(x) of src/recursive/prefix_orbit.rs:132-136,
 * std's DefaultHasher (SipHash-1-3, keys 0, 0) over the usize's 8 little-endian bytes.
 * Errors as ans_cat_push / ans_cat_pop (ANS_E_SYMBOL, ANS_E_ZERO_MASS, ANS_E_EXHAUSTED); a table
 * of more than 65,536 symbols, or one in which two symbols share an orbit id, is ANS_E_ARG.
 * Any message, any tail generator.  It saves log2(n! / prod multiplicity!) bits over ans_push_iid. */
uint64_t ans_orbit_id(uint64_t x);
int ans_mset_push(ans_msg *m, const ans_table *t, const uint32_t *syms, size_t n);
int ans_mset_pop(ans_msg *m, const ans_table *t, uint32_t *out, size_t n);
/* The Pólya urn model of one undirected graph's edge set: multiset_shuffle_codec(
 * PolyaUrnEdgeIndicesCodec<Undirected>{num_nodes, num_edges, loops, redraws}), the harness's
 * polya_urn(n, E, loops, redraws)  src/graph_codec.rs:210-375, src/recursive/multiset.rs:126-136.
 * edges: num_edges distinct uint32 pairs (i, j) with i <= j < num_nodes (the alphabet of section 5);
 * fewer than 2^31 of them.  The order of the pairs does not matter to push.
 *   push: E <= 11 is plain_shuffle_codec (src/plain/mod.rs:111-116): the pairs sorted as tuples, a
 *         permutation POPPED by PermutationUniform{E}, the permuted vector pushed by the ordered
 *         codec.  E >= 12 is the joint recursive codec (src/recursive/mod.rs:117-134, joint.rs):
 *         for L = E .. 1 an orbit is popped under the L pairs left (orbit id = hash((i, j)), every
 *         orbit a singleton) and swapped to position L - 1; then the ordered push.
 *         The ordered codec (src/graph_codec.rs:318-326) removes the pairs last to first; each is
 *         pushed by the per-edge plain shuffle (:269-276) under the urn over the nodes with mass
 *         degree + 1: the second node with the first node's own mass taken out unless `loops`, and
 *         its current neighbours' unless `redraws`; then the first node.
 *   pop:  the inverse.  E <= 11 returns the pairs sorted, E >= 12 in pop order (deterministic).
 * ANS_E_SYMBOL: i > j, a node >= num_nodes, a loop without `loops`, a pair given (or decoded) twice.
 * ANS_E_ZERO_MASS: a pop whose urn is empty after the exclusions.  ANS_E_EXHAUSTED: as ans_cat_pop.
 * ANS_E_ARG: 2^31 or more pairs, or two different pairs with one orbit id (not built).
 * The orbit id is SipHash-1-3, keys 0, 0, over the two usizes' 16 bytes (csrc/ans_polya.hpp edge_id).
 * A failed call leaves the message wherever the failing step found it.  Directed graphs are not
 * coded (the reference asserts !is_directed, :220). */
int ans_polya_push(ans_msg *m, uint32_t num_nodes, int loops, int redraws, const uint32_t *edges, size_t num_edges);
int ans_polya_pop(ans_msg *m, uint32_t num_nodes, int loops, int redraws, uint32_t *edges, size_t num_edges);
/* One undirected, unlabelled graph under the autoregressive Erdős–Rényi model, as a labelled graph
 * or up to the order of its nodes: Autoregressive(ErdosRenyiSliceCodecs) (src/recursive/mod.rs:190-216,
 * src/recursive/graph/slice.rs:16-59; the harness's ord_AE) and ShuffleCodec<ErdosRenyiSliceCodecs,
 * WLOrbitCodecs<GraphPrefix>> with wl_iter = 0 (src/recursive/mod.rs:117-148, src/recursive/graph/
 * incomplete.rs:189-236; the harness's wl0r_AE with the extra half iteration, wl0-r_AE without).
 * edges: num_edges distinct uint32 pairs (i, j) with i <= j < num_nodes, fewer than 2^31 of them, in
 * any order.  bern: a table of exactly two symbols, [norm - mass, mass] (ans_table_create_bernoulli);
 * symbol 1 says "the pair is an edge".  The slice of position v is the 0/1 vector over (v, v+1) ..
 * (v, num_nodes-1), then (v, v) when `loops`, coded as IID<Bernoulli>: pushed last entry first.
 *   orbits = ANS_ORBITS_NONE:      push codes slice num_nodes-1 .. 0, pop decodes slice 0 .. num_nodes-1;
 *                                  the decoded graph is the input.
 *   orbits = ANS_ORBITS_DEGREE:    the class of a known node is its degree in the whole graph (a loop
 *                                  counts once), classes in ascending order of their id, SipHash-1-3
 *                                  (keys 0, 0) over the 16 bytes (ans_orbit_id(0), degree).
 *                                  push: for L = num_nodes .. 1 a class is POPPED under the counts of
 *                                  the classes at positions < L (norm L), its smallest position and
 *                                  position L - 1 change nodes, and slice L - 1 is pushed.
 *                                  pop: for v = 0 .. num_nodes-1 slice v is popped and the class of
 *                                  position v is PUSHED under the counts of positions <= v.
 *                                  The decoded graph is the input relabelled by the permutation the
 *                                  push chose.  Saves log2(n! / prod c_k!) bits, c_k the number of
 *                                  nodes of the k-th distinct degree.
 *   orbits = ANS_ORBITS_ONE_CLASS: the same with every known node in one class (saves nothing).
 * push: perm is NULL or receives num_nodes entries, perm[position] = the input node there (the
 * identity for NONE).  pop: edges receives the pairs (v, w), v <= w, as positions, in pop order (v
 * ascending, within v the slice's order, the loop last), *num_edges their number; more than cap
 * of them is ANS_E_LEN.
 * ANS_E_SYMBOL: i > j, a node >= num_nodes, a loop without `loops`, a pair given twice.
 * ANS_E_ZERO_MASS: a needed symbol of mass 0, as ans_cat_push.  ANS_E_EXHAUSTED: as ans_cat_pop.
 * ANS_E_ARG: a table without exactly two symbols, an `orbits` outside the three values, 2^31 or
 * more pairs or nodes, or two degrees <= num_nodes with one class id (none below 70,000).
 * A failed call leaves the message wherever the failing step found it.  Deeper WL iterations are
 * ans_ar_er_wl_push / _pop below; labels and directed graphs are not coded;
 * PolyaUrnSliceCodecs is ans_ar_polya_push / _pop below. */
#define ANS_ORBITS_NONE 0
#define ANS_ORBITS_ONE_CLASS 1
#define ANS_ORBITS_DEGREE 2
int ans_ar_er_push(ans_msg *m, const ans_table *bern, uint32_t num_nodes, int loops, int orbits,
                   const uint32_t *edges, size_t num_edges, uint32_t *perm /* NULL, or num_nodes out */);
int ans_ar_er_pop(ans_msg *m, const ans_table *bern, uint32_t num_nodes, int loops, int orbits, uint32_t *edges,
                  size_t cap, size_t *num_edges);
/* The same graph under the autoregressive Pólya urn model: Autoregressive(PolyaUrnSliceCodecs)
 * (src/recursive/graph/slice.rs:61-230; the harness's ord_AP) and ShuffleCodec<PolyaUrnSliceCodecs,
 * WLOrbitCodecs<GraphPrefix>> with wl_iter = 0 (wl0r_AP / wl0-r_AP).  edges, perm, `orbits` and the
 * order of the steps are those of ans_ar_er_push / _pop; only the slice's codec differs.  The slice of
 * position v is the SET of its pairs (v, j), j among the unknown positions v+1 .. num_nodes-1 and v
 * itself when `loops`, s_v = num_nodes - v - 1 + loops of them:
 *   its size len under LogUniform(bitlen(s_v) + 1): b = bitlen(len) under Uniform(bitlen(s_v) + 2),
 *   below it len - 2^(b-1) under Uniform(2^(b-1)) when b > 0;
 *   if len > 0, multiset_shuffle_codec over the pairs (plain for len <= 11, joint with the orbit id
 *   SipHash-1-3 of (v, j) beyond, as ans_polya_push) around the ordered codec: the j's are drawn
 *   without replacement from the urn over the positions v + !loops .. num_nodes-1, mass(j) = 1 + the
 *   number of j's neighbours among the positions < v (a loop counts once).
 * pop: edges receives the pairs (v, w), v <= w, as positions: v ascending, within v by w ascending
 * (the loop first), *num_edges their number; more than cap of them is ANS_E_LEN.
 * ANS_E_SYMBOL: as ans_ar_er_push; pop: a decoded slice size above s_v (bytes no push wrote).
 * ANS_E_ARG: an `orbits` outside the three values, 2^31 or more pairs or nodes, two degrees with one
 * class id, or two pairs of one slice of 12 or more with one orbit id.  ANS_E_EXHAUSTED: as ans_cat_pop. */
int ans_ar_polya_push(ans_msg *m, uint32_t num_nodes, int loops, int orbits, const uint32_t *edges,
                      size_t num_edges, uint32_t *perm /* NULL, or num_nodes out */);
int ans_ar_polya_pop(ans_msg *m, uint32_t num_nodes, int loops, int orbits, uint32_t *edges, size_t cap,
                     size_t *num_edges);
/* The same two codecs up to the order of the nodes with Weisfeiler-Lehman orbits of any depth:
 * ShuffleCodec<.., WLOrbitCodecs<GraphPrefix>> with num_iter = wl_iter (0 .. ANS_WL_MAX_ITER, else
 * ANS_E_ARG) and extra_half_iter = half_iter (src/recursive/graph/incomplete.rs:45-57, 87-151,
 * 189-236; the harness's wl<k>r_AE / wl<k>r_AP with the half iteration, wl<k>-r_.. without; its
 * default is wl_iter 1 with the half iteration).  The steps, the slices, edges, perm, the order of
 * the popped pairs and the statuses are those of ans_ar_er_push / _pop and ans_ar_polya_push / _pop
 * under ANS_ORBITS_DEGREE; only the class of a known position differs.  With hash(words) =
 * SipHash-1-3, keys 0, 0, over 8-byte words, deg(i) the neighbours of position i in the prefix
 * graph (every edge with a known end; a loop counts once and makes its node its own neighbour):
 *   h_0(i) = hash(0) for a known position, hash(1, i) for an unknown one; with half_iter then
 *            hash(h_0(i), deg(i));
 *   h_t+1(i) = hash(h_t(i), deg(i), h_t(j) for j adjacent to i in ascending order), t < wl_iter;
 *   the class of i is the vector h_0(i) .. h_wl_iter(i), classes in ascending lexicographic order.
 * wl_iter = 0 gives the bytes of ANS_ORBITS_DEGREE (half_iter) and ANS_ORBITS_ONE_CLASS (without).
 * ANS_E_ARG also for 2 (wl_iter + 1) num_nodes >= 2^32 (the id words of a graph are indexed by 32 bits).
 * The ids are carried from step to step (recomputed within distance wl_iter of a slice's nodes) and
 * equal WLOrbitCodecs::apply of the prefix at every step.  Labels and directed graphs are not coded
 * (DESIGN.md section 5). */
#define ANS_WL_MAX_ITER 3
int ans_ar_er_wl_push(ans_msg *m, const ans_table *bern, uint32_t num_nodes, int loops, int wl_iter, int half_iter,
                      const uint32_t *edges, size_t num_edges, uint32_t *perm /* NULL, or num_nodes out */);
int ans_ar_er_wl_pop(ans_msg *m, const ans_table *bern, uint32_t num_nodes, int loops, int wl_iter, int half_iter,
                     uint32_t *edges, size_t cap, size_t *num_edges);
int ans_ar_polya_wl_push(ans_msg *m, uint32_t num_nodes, int loops, int wl_iter, int half_iter,
                         const uint32_t *edges, size_t num_edges, uint32_t *perm /* NULL, or num_nodes out */);
int ans_ar_polya_wl_pop(ans_msg *m, uint32_t num_nodes, int loops, int wl_iter, int half_iter, uint32_t *edges,
                        size_t cap, size_t *num_edges);
/* Joint shuffle coding of the same graph: ShuffleCodec<JointSliceCodecs<C>, WLOrbitCodecs<JointPrefix<_>>>
 * (src/recursive/joint.rs, src/recursive/mod.rs:117-148, src/recursive/graph/incomplete.rs:154-187,
 * src/graph_codec.rs:405-450).  The graph is coded whole by an ordered codec C and the order of its
 * nodes is taken back through the orbit codecs above.  push: the ids of the full graph; num_nodes times
 * the blanket pop of a class under norm len, its smallest position swapped with position len - 1, which
 * leaves the known ones, and the ids updated around it; then C pushes the permuted graph.  pop: C's
 * graph, the ids with every position unknown, then num_nodes times a position joins, the ids are
 * updated around it and its class is pushed.  The classes are those of ans_ar_er_wl_push with two
 * differences: the prefix graph keeps every edge (a neighbour counts even when both ends are unknown,
 * deg(i) is the full degree), and only the position that changed sides is at distance 0 of an update.
 * perm and the statuses are those of ans_ar_er_wl_push / _pop.  A failed call leaves the message as
 * it found it.
 *   ans_joint_er_wl_*:    C = GraphIID<EmptyCodec, EmptyCodec, ErdosRenyi<Undirected>>, IID<Bernoulli> over
 *     AllEdgeIndices (src/graph_codec.rs:104-139, 184-199): the loops (i, i) by i when `loops`, then
 *     the pairs (i, j), i < j, by j, then by i; the last slot is pushed first.  pop: edges receives
 *     the pairs in that order, *num_edges their number; more than cap of them is ANS_E_LEN.
 *   ans_joint_polya_wl_*: C = polya_urn(num_nodes, num_edges, loops, redraws), ans_polya_push / _pop
 *     unchanged on the pairs of positions.  num_edges is a parameter of the codec: a pop takes it and
 *     edges receives that many pairs as ans_polya_pop gives them. */
int ans_joint_er_wl_push(ans_msg *m, const ans_table *bern, uint32_t num_nodes, int loops, int wl_iter, int half_iter,
                         const uint32_t *edges, size_t num_edges, uint32_t *perm /* NULL, or num_nodes out */);
int ans_joint_er_wl_pop(ans_msg *m, const ans_table *bern, uint32_t num_nodes, int loops, int wl_iter, int half_iter,
                        uint32_t *edges, size_t cap, size_t *num_edges);
int ans_joint_polya_wl_push(ans_msg *m, uint32_t num_nodes, int loops, int redraws, int wl_iter, int half_iter,
                            const uint32_t *edges, size_t num_edges, uint32_t *perm /* NULL, or num_nodes out */);
int ans_joint_polya_wl_pop(ans_msg *m, uint32_t num_nodes, int loops, int redraws, int wl_iter, int half_iter,
                           uint32_t *edges, size_t num_edges);
/* The same two codecs for graphs with node and edge labels: ShuffleCodec<..SliceCodecs<NodeC, EdgeC, _>,
 * WLOrbitCodecs<_, N, E, _>> over Graph<N, E, Undirected> (src/recursive/graph/mod.rs:53-104,
 * slice.rs:33-51, 185-192, src/graph_codec.rs:58-94, incomplete.rs:45-57, 97-151, 193-210).  A label
 * is a usize under a Categorical: `node` codes node_labels (num_nodes entries by input node), `edge`
 * codes edge_labels (entry k the label of pair k).  A NULL table is EmptyCodec: that label is absent,
 * is not coded and feeds no hash; its array must then be NULL too, and a table without its array
 * is ANS_E_ARG.  With both NULL the bytes are those of ans_ar_er_wl_push / ans_ar_polya_wl_push.
 * The slice of position v is (its label, the pairs (v, j) with their labels) under the tuple
 * (NodeC, EdgesIID<EdgeC, indices>), which pushes .1 first: a push of a slice pushes the pairs'
 * labels in descending order of j (j the position after the step's swap; IID pops them ascending),
 * then the indices as above, then the node's label; a pop takes the node's label, the indices, sorts
 * them ascending, then takes a label per index.  In the class of a position, with E(i) the labels of
 * i's pairs in the prefix graph:
 *   h_0(i) = hash(label(i), 0) for a known position, hash(0, 1, i) for an unknown one (pop_slice took
 *            its label out) when nodes carry labels, else as above; with half_iter then
 *            hash(h_0(i), deg(i), E(i) ascending) when edges carry labels, else as above;
 *   h_t+1(i) = hash(h_t(i), deg(i), (h_t(j), label(i, j)) for j adjacent to i, the pairs ascending
 *            lexicographically, two words each) when edges carry labels, else as above.
 * pop: node_labels receives the label of every position, edges the pairs (v, w) as positions, v
 * ascending and within v w ascending (the loop first, under either slice model), edge_labels[k] the
 * label of pair k of edges; the popped graph is the input relabelled by the push's perm.
 * ANS_E_SYMBOL: a label outside its table; ANS_E_ZERO_MASS: a label of mass 0 (both before a byte
 * of the message moves); ANS_E_NORM_RANGE: a table whose masses sum to 0.  Else as above. */
int ans_ar_er_wl_labelled_push(ans_msg *m, const ans_table *bern, uint32_t num_nodes, int loops, int wl_iter,
                               int half_iter, const uint32_t *edges, size_t num_edges,
                               uint32_t *perm /* NULL, or num_nodes out */, const ans_table *node /* or NULL */,
                               const ans_table *edge /* or NULL */, const uint32_t *node_labels,
                               const uint32_t *edge_labels);
int ans_ar_er_wl_labelled_pop(ans_msg *m, const ans_table *bern, uint32_t num_nodes, int loops, int wl_iter,
                              int half_iter, uint32_t *edges, size_t cap, size_t *num_edges,
                              const ans_table *node /* or NULL */, const ans_table *edge /* or NULL */,
                              uint32_t *node_labels /* num_nodes out */, uint32_t *edge_labels /* cap out */);
int ans_ar_polya_wl_labelled_push(ans_msg *m, uint32_t num_nodes, int loops, int wl_iter, int half_iter,
                                  const uint32_t *edges, size_t num_edges, uint32_t *perm, const ans_table *node,
                                  const ans_table *edge, const uint32_t *node_labels, const uint32_t *edge_labels);
int ans_ar_polya_wl_labelled_pop(ans_msg *m, uint32_t num_nodes, int loops, int wl_iter, int half_iter,
                                 uint32_t *edges, size_t cap, size_t *num_edges, const ans_table *node,
                                 const ans_table *edge, uint32_t *node_labels, uint32_t *edge_labels);

/* ======================================================================
 * (4) GPU bulk path (MI355X / gfx950) — the data-parallel hot path.
 *     n symbols are cut into chunks of chunk_len (the last may be shorter); chunk j is
 *     ONE independent reference message: Message::zeros(), IID<Categorical>::push of
 *     its symbols (src/codec.rs:415-420, src/ans.rs:96-105), flatten (src/ans.rs:255).
 *     Its stream is byte-identical to that.  Decode is IID::pop on
 *     Message::unflatten(stream) (src/codec.rs:422-424, src/ans.rs:107-116,262).
 *     Symbols are unsigned integers of sym_bytes = 1, 2 or 4 bytes.
 *     Tables with 1 <= nsym <= 65536 and norm < 2^32 take the table kernels; larger ones the
 *     exact 64-bit kernels of section 4b (norm <= 2^56, else ANS_E_NORM_RANGE).
 * ====================================================================== */
typedef struct ans_gpu ans_gpu;
typedef struct ans_gpu_table ans_gpu_table;

int ans_gpu_device_count(int *count);
/* one context per device; owns a HIP stream */
int ans_gpu_create(int device, ans_gpu **out);
void ans_gpu_free(ans_gpu *g);
/* Page-locked host memory for the host-buffer calls below (hipHostMalloc): their copies
 * then run asynchronously and overlap; pageable buffers go through the runtime's staging. */
int ans_host_alloc(size_t bytes, void **out);
void ans_host_free(void *p);
/* Symbol bytes per batch of the host-buffer pipeline below (0 = the default, 128 MiB).
 * Batches overlap their H2D copy, kernels and D2H copy on separate streams. */
int ans_gpu_set_batch_bytes(ans_gpu *g, uint64_t batch_bytes);
/* The pipeline's workspace slots: 0 until the first host-buffer call builds the pipeline, then
 * ANS_PIPE_DEPTH as read at that moment (2..8; default 6). */
int ans_gpu_pipe_depth(const ans_gpu *g, int *depth);
/* uploads the table (and its derived reciprocal / icdf-bucket data) to the device */
int ans_gpu_table_create(ans_gpu *g, const ans_table *t, ans_gpu_table **out);
void ans_gpu_table_free(ans_gpu_table *gt);
/* Which kernels full chunks of this table take (bit flags; chunks outside them, e.g. a ragged
 * last chunk, take the generic one-lane-per-chunk kernels): */
#define ANS_PATH_ENC_LDS 1u     /* fast encoder, rows staged in LDS (<= 256 symbols) */
#define ANS_PATH_ENC_GLOBAL 2u  /* fast encoder, rows read from global memory (larger alphabets) */
#define ANS_PATH_DEC_LDS 4u     /* fast decoder, icdf buckets in LDS */
#define ANS_PATH_DEC_GLOBAL 8u  /* fast decoder, icdf buckets in global memory */
#define ANS_PATH_ENC_WIDE 16u   /* large alphabet, norm >= 2^22: cdf-pair rows, LDS prefix (128-B symbol groups) */
#define ANS_PATH_DEC_WIDE 32u   /* large alphabet: LDS prefix icdf + global buckets */
#define ANS_PATH_DEC_COMPACT 64u /* ... whose global buckets are 16 B (u16 candidate offsets) */
#define ANS_PATH_ENC_PACKED 128u /* large-alphabet encoder with the packed (u32 base + u16) LDS prefix */
#define ANS_PATH_DEC_U 256u     /* LDS decoder without the quotient fix-up (u-domain tables): applies to
                                  * sym_bytes == 1 only; u16 / u32 decodes of the same table run the
                                  * row decoder (kModeRows: the same bytes, one fix-up more) */
#define ANS_PATH_ENC_SHIFT 512u /* packed large-alphabet encoder whose renorm reads a shift byte per
                                  * mass (every mass <= 4096) instead of comparing bit lengths */
int ans_gpu_table_paths(const ans_gpu_table *gt, uint32_t *paths);
/* Which coder kernels the context's last launcher call started, in launch order, each with every
 * template argument its launch ladder chose, as text joined by ';':
 *   k_encode<u8,kmax=2,k32=0,grows=0,var=0,nr=std,m24=1>;k_encode_generic<u8,lds=1,fast=1>
 *   k_decode<u8,spp=16,mode=u,p24=1,j4=0,var=0,nr=std>      (mode: far / rows / u; nr: std / small / big)
 *   k_encode_w<u16,k32=1,pack=1,sa=1,var=0,nr=std>   k_decode_w<u16,compact=1,prefix=0,var=0,p24=1,nr=std>
 *   k_decode_g<u16,nr=std>   k_decode_generic<u8,lds=1,fast=1>
 *   k_menc<indep,u8,spp=16,lanes=256,res=0,rare=0,nr=std>   k_mdec<indep,u8,spp=16,lanes=256,res=0,lean=1,nr=std>
 *   k_encode64<catset,u8>   k_decode64<catset,u8>   k_push64<u8>   k_pop64<u8>
 *   k_mset_push<u8,cnt=lds>   k_mset_pop<u16,cnt=global>      (cnt: where the per-lane counts live)
 *   k_polya_push<redraws=0>   k_polya_pop<redraws=1>          (section 5c)
 *   k_arer_push<orbits=2>   k_arer_pop<orbits=0>              (section 5d)
 *   k_arpu_push<orbits=2>   k_arpu_pop<orbits=0>              (section 5e)
 * The calls that write it are the Categorical table's (sections 3 and 4: fixed, ragged and variable
 * chunks, host or device buffers; a pipelined host call leaves its last batch's launches), the
 * Independent ones (new messages and resume), the multiset ones, the Pólya urn ones and the autoregressive Erdős–Rényi and Pólya urn ones; helper kernels (staging, compaction) are not named,
 * and the other calls (and calls that return before any launch: no symbols, bad arguments) leave
 * the record as it was.  Empty before the first such call.
 * Writes *len = the text's bytes (without the terminating NUL) and, if cap > *len, the
 * NUL-terminated text into buf; a shorter buf (or buf == NULL) is ANS_E_LEN with *len set.
 * For tests and tuning: the text is not a stable interface. */
int ans_gpu_last_launch(const ans_gpu *g, char *buf, size_t cap, size_t *len);
/* The workgroup count of launch `index` (0-based, in launch order) of the same record.  Kept for
 * the kernels whose lanes are bounded by a workspace of the context's, where one lane codes several
 * items in turn: k_mset_push / k_mset_pop (saturating at 32,767: the cnt=lds form launches one
 * lane per chunk), k_polya_push / k_polya_pop, k_arer_push / k_arer_pop and k_arpu_push / k_arpu_pop; *workgroups = 0 for the other kernels, whose
 * records do not keep it.  Lanes = 64 x workgroups.  ANS_E_ARG for an index at or past the
 * launches recorded.  For tests and tuning, as the text is. */
int ans_gpu_last_launch_grid(const ans_gpu *g, uint32_t index, uint32_t *workgroups);
/* worst-case stream bytes of one chunk of chunk_len symbols, rounded up to 16 */
int ans_gpu_slot_capacity(const ans_gpu_table *gt, uint64_t chunk_len, uint64_t *slot_cap);

/* Host buffers in, host buffers out (synchronous; includes H2D/D2H), pipelined in batches
 * of chunks over a persistent device workspace.  Page-locked host buffers let the copies
 * run asynchronously; pageable ones still work (the runtime stages them).
 * Encode writes the streams densely: chunk j at out[offsets[j] .. offsets[j]+lens[j]).
 * out_cap must hold the total (query the exact total by passing out == NULL: *total is
 * set and nothing else is written). */
int ans_gpu_encode_chunks(ans_gpu_table *gt, const void *syms, int sym_bytes, uint64_t n, uint64_t chunk_len,
                          uint8_t *out, uint64_t out_cap, uint64_t *offsets, uint64_t *lens, uint64_t *total);
/* gen_kind = ANS_GEN_ZEROS or ANS_GEN_EMPTY (what an exhausted stream yields); returns
 * ANS_E_MISMATCH if a chunk does not return to Message::zeros() (src/ans.rs:56). */
int ans_gpu_decode_chunks(ans_gpu_table *gt, const uint8_t *in, uint64_t in_len, const uint64_t *offsets,
                          const uint64_t *lens, uint64_t n, uint64_t chunk_len, int gen_kind, void *out,
                          int sym_bytes);

/* Chunks from another initial message (the _ex variants of this section): gen_kind = ANS_GEN_ZEROS
 * (Message::zeros(), what the plain calls use), ANS_GEN_EMPTY (Message::empty(): same bytes, an
 * exhausted tail is ANS_E_EXHAUSTED on decode) or ANS_GEN_RANDOM (chunk c starts from
 * Message::random(seed + c), src/ans.rs:285-290: head 1 then seven generator bytes pulled, the
 * reference harness' initial message, src/multiset.rs:174, src/benchmark.rs:698-700).  A push
 * never pulls, so a chunk's stream holds no generated byte; decode is
 * Message::unflatten(m.flatten()) of that message (src/ans.rs:57: the tail keeps its generator
 * state) and must end back at Message::random(seed + c) (src/ans.rs:56), else ANS_E_MISMATCH.
 * A corrupt RANDOM stream that reaches past its start is reported, not decoded further. */
int ans_gpu_encode_chunks_ex(ans_gpu_table *gt, const void *syms, int sym_bytes, uint64_t n, uint64_t chunk_len,
                             int gen_kind, uint64_t seed, uint8_t *out, uint64_t out_cap, uint64_t *offsets,
                             uint64_t *lens, uint64_t *total);
int ans_gpu_decode_chunks_ex(ans_gpu_table *gt, const uint8_t *in, uint64_t in_len, const uint64_t *offsets,
                             const uint64_t *lens, uint64_t n, uint64_t chunk_len, int gen_kind, uint64_t seed,
                             void *out, int sym_bytes);

/* Device-resident variants: all pointers are device pointers; asynchronous on `stream`
 * (a hipStream_t; NULL = the context's stream).  Streams live in fixed slots: chunk j at
 * d_slots + j*slot_cap (slot_cap from ans_gpu_slot_capacity).  Errors found on the
 * device are OR-ed into *d_status as (1u << status) bits; read with ans_dev_status. */
int ans_dev_encode_chunks(ans_gpu_table *gt, const void *d_syms, int sym_bytes, uint64_t n, uint64_t chunk_len,
                          uint8_t *d_slots, uint64_t slot_cap, uint32_t *d_lens, uint32_t *d_status, void *stream);
/* d_offsets == NULL: chunk j's stream starts at d_in + j*slot_cap (the encoder's layout);
 * otherwise at d_in + d_offsets[j] (e.g. a dense container, at any alignment: the fast decoders
 * read it in place).  The fast decoders (k_decode, k_decode_w) read no byte outside the
 * stream; k_decode_g (norm < 2^22 with more than 256 symbols) may read every byte of the
 * aligned 128-B lines holding a stream, so such a container needs 128 readable bytes past its end.
 * A d_lens entry above slot_cap (slot layout) or of 2^27 bytes or more (no stream of a chunk
 * the fast decoders take reaches that) is foreign or corrupt: ANS_E_LEN. */
int ans_dev_decode_chunks(ans_gpu_table *gt, const uint8_t *d_in, const uint64_t *d_offsets, uint64_t slot_cap,
                          const uint32_t *d_lens, uint64_t n, uint64_t chunk_len, int gen_kind, void *d_syms,
                          int sym_bytes, uint32_t *d_status, void *stream);
int ans_dev_encode_chunks_ex(ans_gpu_table *gt, const void *d_syms, int sym_bytes, uint64_t n, uint64_t chunk_len,
                             int gen_kind, uint64_t seed, uint8_t *d_slots, uint64_t slot_cap, uint32_t *d_lens,
                             uint32_t *d_status, void *stream);
int ans_dev_decode_chunks_ex(ans_gpu_table *gt, const uint8_t *d_in, const uint64_t *d_offsets, uint64_t slot_cap,
                             const uint32_t *d_lens, uint64_t n, uint64_t chunk_len, int gen_kind, uint64_t seed,
                             void *d_syms, int sym_bytes, uint32_t *d_status, void *stream);
/* Synthetic iid symbols, counter-based: symbol i of seed k is
 * icdf(floor(splitmix64((k << 48) ^ (start + i)) * norm / 2^64)). */
int ans_dev_gen_iid(ans_gpu_table *gt, uint64_t seed, uint64_t start, uint64_t n, void *d_syms, int sym_bytes,
                    void *stream);
/* Codec::samples (src/ans.rs:38-44) in bulk: chunk c of chunk_len symbols (the last may be
 * shorter) is IID::new(codec, len).sample(seed + c), i.e. len pops from
 * Message::random(seed + c).  The Random generator restates rand_pcg 0.3.1 Pcg64Mcg /
 * rand_core 0.6 seed_from_u64 / rand 0.8.5 (bytes parity-unpinned: no reference test pins
 * them), identically to the host's ANS_GEN_RANDOM. */
int ans_dev_sample_iid(ans_gpu_table *gt, uint64_t seed, uint64_t n, uint64_t chunk_len, void *d_syms, int sym_bytes,
                       void *stream);
int ans_gpu_sample_iid(ans_gpu_table *gt, uint64_t seed, uint64_t n, uint64_t chunk_len, void *out, int sym_bytes);
/* Variable-length chunks: chunk c is symbols [starts[c], starts[c+1]) (nchunks + 1
 * non-decreasing entries), still one reference message each, e.g. one graph or one record per
 * chunk.  One lane per chunk; slot_cap = ans_gpu_slot_capacity of the longest chunk.  Symbols
 * live at their absolute index (the buffers span [0, starts[nchunks])).  The chunks are staged
 * for the fast kernels when the padded layout stays within twice the symbols plus 64 MiB (else
 * the generic kernels); the ans_dev_ entries find the longest chunk on the device, which costs
 * one 16-byte copy back and a synchronisation of `stream` before the kernels are queued. */
int ans_dev_encode_var_chunks(ans_gpu_table *gt, const void *d_syms, int sym_bytes, uint64_t nchunks,
                              const uint64_t *d_starts, uint8_t *d_slots, uint64_t slot_cap, uint32_t *d_lens,
                              uint32_t *d_status, void *stream);
/* d_offsets == NULL: chunk c's stream at d_in + c*slot_cap; else at d_in + d_offsets[c] */
int ans_dev_decode_var_chunks(ans_gpu_table *gt, const uint8_t *d_in, const uint64_t *d_offsets, uint64_t slot_cap,
                              const uint32_t *d_lens, uint64_t nchunks, const uint64_t *d_starts, int gen_kind,
                              void *d_syms, int sym_bytes, uint32_t *d_status, void *stream);
int ans_gpu_encode_var_chunks(ans_gpu_table *gt, const void *syms, int sym_bytes, uint64_t nchunks,
                              const uint64_t *starts, uint8_t *out, uint64_t out_cap, uint64_t *offsets,
                              uint64_t *lens, uint64_t *total);
int ans_gpu_decode_var_chunks(ans_gpu_table *gt, const uint8_t *in, uint64_t in_len, const uint64_t *offsets,
                              const uint64_t *lens, uint64_t nchunks, const uint64_t *starts, int gen_kind, void *out,
                              int sym_bytes);
/* ... from the initial messages of the _ex note above (chunk c: Message::random(seed + c)) */
int ans_dev_encode_var_chunks_ex(ans_gpu_table *gt, const void *d_syms, int sym_bytes, uint64_t nchunks,
                                 const uint64_t *d_starts, int gen_kind, uint64_t seed, uint8_t *d_slots,
                                 uint64_t slot_cap, uint32_t *d_lens, uint32_t *d_status, void *stream);
int ans_dev_decode_var_chunks_ex(ans_gpu_table *gt, const uint8_t *d_in, const uint64_t *d_offsets, uint64_t slot_cap,
                                 const uint32_t *d_lens, uint64_t nchunks, const uint64_t *d_starts, int gen_kind,
                                 uint64_t seed, void *d_syms, int sym_bytes, uint32_t *d_status, void *stream);
int ans_gpu_encode_var_chunks_ex(ans_gpu_table *gt, const void *syms, int sym_bytes, uint64_t nchunks,
                                 const uint64_t *starts, int gen_kind, uint64_t seed, uint8_t *out, uint64_t out_cap,
                                 uint64_t *offsets, uint64_t *lens, uint64_t *total);
int ans_gpu_decode_var_chunks_ex(ans_gpu_table *gt, const uint8_t *in, uint64_t in_len, const uint64_t *offsets,
                                 const uint64_t *lens, uint64_t nchunks, const uint64_t *starts, int gen_kind,
                                 uint64_t seed, void *out, int sym_bytes);
/* Device-resident dense container (the wire format ans_gpu_encode_chunks returns): the chunks
 * are encoded into d_slots (scratch, nchunks * slot_cap bytes), their lengths scanned into
 * d_offsets and the streams packed: chunk j at d_out[d_offsets[j] .. + d_lens[j]),
 * d_offsets[nchunks] = the total.  d_offsets holds ans_dense_offsets_entries(nchunks) entries
 * (those past nchunks + 1 are scratch).  d_out must hold the total (nchunks * slot_cap always
 * does); a stream that would end past out_cap is not written and sets ANS_E_LEN in *d_status.
 * Asynchronous on `stream`.  ans_dev_decode_chunks(_ex) reads the container in place (the
 * fast decoders fetch the aligned 128-B lines around each stream).  Replaces the encode side of
 * src/codec.rs:411-419 IID::push over many messages plus their concatenation. */
uint64_t ans_dense_offsets_entries(uint64_t nchunks);
int ans_dev_encode_dense(ans_gpu_table *gt, const void *d_syms, int sym_bytes, uint64_t n, uint64_t chunk_len,
                         uint8_t *d_slots, uint64_t slot_cap, uint32_t *d_lens, uint64_t *d_offsets, uint8_t *d_out,
                         uint64_t out_cap, uint32_t *d_status, void *stream);
int ans_dev_encode_dense_ex(ans_gpu_table *gt, const void *d_syms, int sym_bytes, uint64_t n, uint64_t chunk_len,
                            int gen_kind, uint64_t seed, uint8_t *d_slots, uint64_t slot_cap, uint32_t *d_lens,
                            uint64_t *d_offsets, uint8_t *d_out, uint64_t out_cap, uint32_t *d_status, void *stream);
/* Compacts slot streams into a dense buffer: d_out[d_offsets[j] ..] = slot j. */
int ans_dev_compact(ans_gpu *g, const uint8_t *d_slots, uint64_t slot_cap, const uint32_t *d_lens,
                    const uint64_t *d_offsets, uint64_t nchunks, uint8_t *d_out, void *stream);
/* The inverse of ans_dev_compact: dense-container streams into the slot layout (which the
 * fast decode kernels read). */
int ans_dev_expand(ans_gpu *g, const uint8_t *d_in, const uint64_t *d_offsets, const uint32_t *d_lens,
                   uint64_t nchunks, uint8_t *d_slots, uint64_t slot_cap, void *stream);
/* Test hook: the fast decoders' renorm step (renorm_up, src/ans.rs:239-243, with the next four
 * stream bytes in the window, first byte on top) on n caller-chosen (head, window) pairs:
 * resulting heads and byte counts.  Heads must be >= 2^24 (at most four bytes pulled). */
int ans_dev_check_renorm(ans_gpu *g, const uint64_t *d_heads, const uint32_t *d_windows, uint64_t L, uint64_t n,
                         uint64_t *d_out_heads, uint32_t *d_out_k, void *stream);
/* Synchronises `stream` and maps the device status word to the lowest set status. */
int ans_dev_status(ans_gpu *g, const uint32_t *d_status, void *stream, int *status);

/* ======================================================================
 * (4b) The other static codecs of src/codec.rs in bulk, one lane per chunk; chunk c is one
 *      reference message from the initial message gen_kind / seed gives it, as in the _ex calls
 *      of section 4.  sym_bytes may also be 8 here.  Fixed chunks whose symbols are whole 128-B
 *      lines (chunk_len * sym_bytes % 128 == 0) run their full chunks on the fast kernels
 *      (ans_mfast.hpp: LDS stream rings, f64 / magic-reciprocal division); the ragged last chunk,
 *      variable chunks, other layouts and Independent sets beyond the fast range run on the
 *      exact 64-bit kernels.  Both give the same bytes.
 *      A Categorical with norm >= 2^32 (up to 2^56) or more than 65536 symbols takes these
 *      kernels through the section-4 calls themselves (ans_gpu_table_create accepts it; its
 *      paths flags are 0; ans_dev_gen_iid / sample_iid return ANS_E_NORM_RANGE for it).
 * ====================================================================== */
/* IID<Uniform(size)>  src/codec.rs:13-49; size <= MAX_SIZE = 2^46 (src/ans.rs:22, ANS_E_NORM_RANGE
 * beyond).  A symbol >= size is ANS_E_SYMBOL (the reference does not check it and codes garbage). */
int ans_gpu_uniform_encode_chunks(ans_gpu *g, uint64_t size, const void *syms, int sym_bytes, uint64_t n,
                                  uint64_t chunk_len, int gen_kind, uint64_t seed, uint8_t *out, uint64_t out_cap,
                                  uint64_t *offsets, uint64_t *lens, uint64_t *total);
int ans_gpu_uniform_decode_chunks(ans_gpu *g, uint64_t size, const uint8_t *in, uint64_t in_len,
                                  const uint64_t *offsets, const uint64_t *lens, uint64_t n, uint64_t chunk_len,
                                  int gen_kind, uint64_t seed, void *out, int sym_bytes);
/* IID<LogUniform::new(excl_max_bits)>  src/codec.rs:561-611 (excl_max_bits <= 64): per symbol a
 * Uniform(2^(bits-1)) push of its low bits, then Uniform(excl_max_bits + 1) of bits = 64 - clz(x);
 * MaxBenfordIID's item (src/param_codec.rs:117-119).  bits > excl_max_bits is ANS_E_SYMBOL,
 * x >= 2^47 is ANS_E_NORM_RANGE (Uniform::new's assert).  A chunk whose pushes would draw from
 * the tail generator (the tail's num_generated, which no byte container carries) is
 * ANS_E_MISMATCH. */
int ans_gpu_loguniform_encode_chunks(ans_gpu *g, uint32_t excl_max_bits, const void *syms, int sym_bytes, uint64_t n,
                                     uint64_t chunk_len, int gen_kind, uint64_t seed, uint8_t *out, uint64_t out_cap,
                                     uint64_t *offsets, uint64_t *lens, uint64_t *total);
int ans_gpu_loguniform_decode_chunks(ans_gpu *g, uint32_t excl_max_bits, const uint8_t *in, uint64_t in_len,
                                     const uint64_t *offsets, const uint64_t *lens, uint64_t n, uint64_t chunk_len,
                                     int gen_kind, uint64_t seed, void *out, int sym_bytes);
/* Independent<Categorical>  src/codec.rs:366-403: position k codes with table table_ids[k] of the set
 * (the Categoricals uploaded once; norms up to 2^56).  Chunk c = positions [c*chunk_len, ...). */
typedef struct ans_gpu_tableset ans_gpu_tableset;
int ans_gpu_tableset_create(ans_gpu *g, const ans_table *const *tables, uint32_t ntables, ans_gpu_tableset **out);
void ans_gpu_tableset_free(ans_gpu_tableset *ts);
int ans_gpu_independent_encode_chunks(ans_gpu_tableset *ts, const uint32_t *table_ids, const void *syms, int sym_bytes,
                                      uint64_t n, uint64_t chunk_len, int gen_kind, uint64_t seed, uint8_t *out,
                                      uint64_t out_cap, uint64_t *offsets, uint64_t *lens, uint64_t *total);
int ans_gpu_independent_decode_chunks(ans_gpu_tableset *ts, const uint32_t *table_ids, const uint8_t *in,
                                      uint64_t in_len, const uint64_t *offsets, const uint64_t *lens, uint64_t n,
                                      uint64_t chunk_len, int gen_kind, uint64_t seed, void *out, int sym_bytes);
/* Independent<Categorical> over variable-length chunks: chunk c is positions [starts[c], starts[c+1])
 * (nchunks + 1 non-decreasing entries; table_ids / syms / out span [0, starts[nchunks])), one
 * reference message each, e.g. one record of mixed fields per chunk.  These run on the exact
 * 64-bit kernels (one lane per chunk), which take any chunk length. */
int ans_gpu_independent_encode_var_chunks(ans_gpu_tableset *ts, const uint32_t *table_ids, const void *syms,
                                          int sym_bytes, uint64_t nchunks, const uint64_t *starts, int gen_kind,
                                          uint64_t seed, uint8_t *out, uint64_t out_cap, uint64_t *offsets,
                                          uint64_t *lens, uint64_t *total);
int ans_gpu_independent_decode_var_chunks(ans_gpu_tableset *ts, const uint32_t *table_ids, const uint8_t *in,
                                          uint64_t in_len, const uint64_t *offsets, const uint64_t *lens,
                                          uint64_t nchunks, const uint64_t *starts, int gen_kind, uint64_t seed,
                                          void *out, int sym_bytes);
/* 1 (fast kernels: every table has <= 256 symbols, the norms all in [2^16, 2^31], all below
 * 2^16 or all in (2^31, 2^32), and at most 15 tables: 257 encoder rows of 32 B per table beside
 * the 32-KiB stream ring in 160 KiB of LDS), 2 (the same, with rows of near-certain symbols that
 * take the voted exact renorm), 0 (exact kernels only: any other set) */
int ans_gpu_tableset_fast(const ans_gpu_tableset *ts, int *fast);
/* The fast kernels' workgroup layout for this set: 0 (default) picks 1,024-lane workgroups
 * sharing one LDS table image (the encoder's when it fits 32 KiB, the decoder's when it fits
 * 28 KiB) for calls of at least (compute units x 1,024) chunks, 256-lane ones below; 256 or
 * 1,024 force one where that image exists (ANS_E_ARG for 1,024 when neither fits).  The bytes
 * are the same either way. */
int ans_gpu_tableset_lanes(ans_gpu_tableset *ts, int lanes);

/* Device-resident 4b calls (replace the bulk IID::push / pop and Independent::push / pop of
 * src/codec.rs:388-399,415-424 on device memory): fixed chunks, chunk j's stream in its slot at
 * d_slots + j*slot_cap (slot_cap from the _slot_capacity calls), lengths in d_lens, errors OR-ed
 * into *d_status as (1u << status) bits (ans_dev_status); asynchronous on `stream` (NULL = the
 * context's).  Decoders read slots (d_offsets NULL) or a dense container at d_in + d_offsets[j].
 * d_tids: the table id of every position, one byte each (sets of at most 256 tables; ids are
 * not range-checked on the device, as the reference would index past its codec vector).
 * slot_cap is the codec's slot capacity (the _slot_capacity call for chunk_len) for every call,
 * dense-container decodes included: it bounds the fast kernels' stream positions, and any other
 * value sends every chunk to the exact kernels.  d_syms, d_tids and d_slots must be 16-byte
 * aligned (the fast kernels move symbols, table ids and slot pages with 16-B vector loads and
 * stores; hipMalloc and torch allocations are); a dense container's streams may start anywhere. */
int ans_gpu_uniform_slot_capacity(uint64_t size, uint64_t chunk_len, uint64_t *slot_cap);
int ans_gpu_loguniform_slot_capacity(uint32_t excl_max_bits, uint64_t chunk_len, uint64_t *slot_cap);
int ans_gpu_tableset_slot_capacity(const ans_gpu_tableset *ts, uint64_t chunk_len, uint64_t *slot_cap);
int ans_dev_uniform_encode(ans_gpu *g, uint64_t size, const void *d_syms, int sym_bytes, uint64_t n, uint64_t chunk_len,
                           int gen_kind, uint64_t seed, uint8_t *d_slots, uint64_t slot_cap, uint32_t *d_lens,
                           uint32_t *d_status, void *stream);
int ans_dev_uniform_decode(ans_gpu *g, uint64_t size, const uint8_t *d_in, const uint64_t *d_offsets, uint64_t slot_cap,
                           const uint32_t *d_lens, uint64_t n, uint64_t chunk_len, int gen_kind, uint64_t seed,
                           void *d_syms, int sym_bytes, uint32_t *d_status, void *stream);
int ans_dev_loguniform_encode(ans_gpu *g, uint32_t excl_max_bits, const void *d_syms, int sym_bytes, uint64_t n,
                              uint64_t chunk_len, int gen_kind, uint64_t seed, uint8_t *d_slots, uint64_t slot_cap,
                              uint32_t *d_lens, uint32_t *d_status, void *stream);
int ans_dev_loguniform_decode(ans_gpu *g, uint32_t excl_max_bits, const uint8_t *d_in, const uint64_t *d_offsets,
                              uint64_t slot_cap, const uint32_t *d_lens, uint64_t n, uint64_t chunk_len, int gen_kind,
                              uint64_t seed, void *d_syms, int sym_bytes, uint32_t *d_status, void *stream);
int ans_dev_independent_encode(ans_gpu_tableset *ts, const uint8_t *d_tids, const void *d_syms, int sym_bytes,
                               uint64_t n, uint64_t chunk_len, int gen_kind, uint64_t seed, uint8_t *d_slots,
                               uint64_t slot_cap, uint32_t *d_lens, uint32_t *d_status, void *stream);
int ans_dev_independent_decode(ans_gpu_tableset *ts, const uint8_t *d_tids, const uint8_t *d_in,
                               const uint64_t *d_offsets, uint64_t slot_cap, const uint32_t *d_lens, uint64_t n,
                               uint64_t chunk_len, int gen_kind, uint64_t seed, void *d_syms, int sym_bytes,
                               uint32_t *d_status, void *stream);
/* ... over variable-length chunks (d_starts: nchunks + 1 device entries; slot_cap from
 * ans_gpu_tableset_slot_capacity of the longest chunk; d_tids one byte per position) */
int ans_dev_independent_encode_var(ans_gpu_tableset *ts, const uint8_t *d_tids, const void *d_syms, int sym_bytes,
                                   uint64_t nchunks, const uint64_t *d_starts, int gen_kind, uint64_t seed,
                                   uint8_t *d_slots, uint64_t slot_cap, uint32_t *d_lens, uint32_t *d_status,
                                   void *stream);
int ans_dev_independent_decode_var(ans_gpu_tableset *ts, const uint8_t *d_tids, const uint8_t *d_in,
                                   const uint64_t *d_offsets, uint64_t slot_cap, const uint32_t *d_lens,
                                   uint64_t nchunks, const uint64_t *d_starts, int gen_kind, uint64_t seed,
                                   void *d_syms, int sym_bytes, uint32_t *d_status, void *stream);

/* Resume: push onto, or pop from, the message ALREADY in each chunk's slot -- the reference's
 * push(&mut Message, x) / pop(&mut Message) on any message (src/ans.rs:96-116), which bits-back
 * coding, codecs of different alphabets composed on one message (GraphIID, src/graph_codec.rs:31-34)
 * and appending to a compressed message rest on.  Chunk c's input message is
 * Message::unflatten(bytes of slot c, d_lens[c] of them) with the Empty tail generator: head 0, so
 * the first operation's renorm_up pulls from the top of the bytes (zero bytes on top of a message
 * are consumed by that pull).  ZEROS and RANDOM tails are out of scope: a byte container cannot carry
 * the tail's num_generated.  A pull past the stream's start sets ANS_E_EXHAUSTED in *d_status and
 * d_lens[c] = 0, and leaves that slot's contents unspecified.
 *   push: Independent::push of the chunk's symbols, last first (src/codec.rs:388-391), then
 *         flatten (src/ans.rs:255-260) back into the slot; d_lens[c] = the new length.
 *   pop:  the chunk's symbols by forward pops (src/codec.rs:393-399) into d_syms, then flatten
 *         of what remains back into the slot; d_lens[c] = the new length.
 * The bytes equal the reference's flatten() byte for byte, the single 0x00 it writes for a head
 * of 0 included: a chunk of zero symbols grows by one zero byte (flatten(unflatten(B)) = B ++ [0]).
 * Push needs slot_cap >= d_lens[c] + ans_gpu_tableset_slot_capacity(ts, chunk_len) (the longest
 * chunk's for _var) to be sure of room; a chunk whose result would pass slot_cap, or whose d_lens[c]
 * is already above it, is ANS_E_LEN with d_lens[c] = 0.  Pop needs slot_cap >= 16 (a result is at
 * most one byte longer than its input).  slot_cap may be any value otherwise, and d_slots at any
 * alignment.  Any set of at most 256 tables, any chunk length, fixed or variable chunks: the exact
 * 64-bit kernels (one lane per chunk) take them all.  ans_dev_independent_push and _pop run their
 * full chunks on the fast kernels instead where ans_gpu_tableset_fast != 0, chunk_len * sym_bytes
 * % 128 == 0, slot_cap % 128 == 0, slot_cap < 2^27 and d_syms, d_tids, d_slots are 16-byte aligned.
 * The ragged last chunk still goes to the exact kernel, and so does a message the fast kernels
 * cannot start from: for a push one too short to fill the 2^56 head (fewer than eight significant
 * bytes), for a pop one with zero bytes on top or too short for the first pull.  Both paths give the
 * same bytes. */
int ans_dev_independent_push(ans_gpu_tableset *ts, const uint8_t *d_tids, const void *d_syms, int sym_bytes,
                             uint64_t n, uint64_t chunk_len, uint8_t *d_slots, uint64_t slot_cap,
                             uint32_t *d_lens /* in/out */, uint32_t *d_status, void *stream);
int ans_dev_independent_pop(ans_gpu_tableset *ts, const uint8_t *d_tids, uint8_t *d_slots /* in/out */,
                            uint64_t slot_cap, uint32_t *d_lens /* in/out */, uint64_t n, uint64_t chunk_len,
                            void *d_syms, int sym_bytes, uint32_t *d_status, void *stream);
int ans_dev_independent_push_var(ans_gpu_tableset *ts, const uint8_t *d_tids, const void *d_syms, int sym_bytes,
                                 uint64_t nchunks, const uint64_t *d_starts, uint8_t *d_slots, uint64_t slot_cap,
                                 uint32_t *d_lens /* in/out */, uint32_t *d_status, void *stream);
int ans_dev_independent_pop_var(ans_gpu_tableset *ts, const uint8_t *d_tids, uint8_t *d_slots /* in/out */,
                                uint64_t slot_cap, uint32_t *d_lens /* in/out */, uint64_t nchunks,
                                const uint64_t *d_starts, void *d_syms, int sym_bytes, uint32_t *d_status,
                                void *stream);
/* ... on host buffers, synchronous: the input messages come as a dense container (chunk c at
 * in[in_offsets[c] .. + in_lens[c]), one entry per chunk) and the results leave as one: chunk c
 * at out[offsets[c] .. + lens[c]).  out == NULL is the size query (*total is set, no container
 * written; pop still fills out_syms); out_cap < *total is ANS_E_LEN.  table_ids are u32 per position
 * as in the calls above. */
int ans_gpu_independent_push_chunks(ans_gpu_tableset *ts, const uint32_t *table_ids, const void *syms, int sym_bytes,
                                    uint64_t n, uint64_t chunk_len, const uint8_t *in, uint64_t in_len,
                                    const uint64_t *in_offsets, const uint64_t *in_lens, uint8_t *out,
                                    uint64_t out_cap, uint64_t *offsets, uint64_t *lens, uint64_t *total);
int ans_gpu_independent_pop_chunks(ans_gpu_tableset *ts, const uint32_t *table_ids, const uint8_t *in, uint64_t in_len,
                                   const uint64_t *in_offsets, const uint64_t *in_lens, uint64_t n, uint64_t chunk_len,
                                   void *out_syms, int sym_bytes, uint8_t *out, uint64_t out_cap, uint64_t *offsets,
                                   uint64_t *lens, uint64_t *total);
int ans_gpu_independent_push_var_chunks(ans_gpu_tableset *ts, const uint32_t *table_ids, const void *syms,
                                        int sym_bytes, uint64_t nchunks, const uint64_t *starts, const uint8_t *in,
                                        uint64_t in_len, const uint64_t *in_offsets, const uint64_t *in_lens,
                                        uint8_t *out, uint64_t out_cap, uint64_t *offsets, uint64_t *lens,
                                        uint64_t *total);
int ans_gpu_independent_pop_var_chunks(ans_gpu_tableset *ts, const uint32_t *table_ids, const uint8_t *in,
                                       uint64_t in_len, const uint64_t *in_offsets, const uint64_t *in_lens,
                                       uint64_t nchunks, const uint64_t *starts, void *out_syms, int sym_bytes,
                                       uint8_t *out, uint64_t out_cap, uint64_t *offsets, uint64_t *lens,
                                       uint64_t *total);

/* Multisets in bulk: ans_mset_push / ans_mset_pop (section 3) of chunk c's symbols as one multiset
 * onto / from the message ALREADY in slot c, one lane per chunk, under the resume contract above word
 * for word: the input is Message::unflatten(slot bytes, d_lens[c]) with the Empty tail, the result is
 * flattened back into the slot and d_lens[c] is its length (a chunk of zero symbols grows by the one
 * 0x00 of flatten); a pull past the stream's start is ANS_E_EXHAUSTED, a result past slot_cap (or a
 * d_lens[c] above it) ANS_E_LEN, a symbol outside the alphabet ANS_E_SYMBOL, one of mass 0
 * ANS_E_ZERO_MASS, each in *d_status with d_lens[c] = 0.  The bytes equal the host codec's.
 * `table` picks the set's table (its alphabet: at most 65,536 symbols, else ANS_E_ARG); sym_bytes is
 * 1, 2 or 4; a chunk holds fewer than 2^32 symbols.  pop writes chunk c's values in pop order at its
 * positions of d_syms.
 * Push needs slot_cap >= d_lens[c] + ans_gpu_tableset_slot_capacity(ts, chunk_len) (the orbit pops
 * only shrink the message).  A pop ends below where it began, but between two steps the message can
 * be longer: step k takes a value's bits out and puts up to log2(k + 1) bits of its orbit back.
 * ans_gpu_mset_pop_slack gives a bound on that growth, (chunk_len / 8 + 1) * ceil(log2(chunk_len + 1))
 * + 16 bytes: with slot_cap >= d_lens[c] + that, a pop never meets ANS_E_LEN (the longest chunk's
 * for _var; the host-buffer calls apply it themselves).
 * The per-lane counts live in LDS as u16 (kernel names k_mset_push<u8,cnt=lds> in ans_gpu_last_launch)
 * when the alphabet has at most 1,024 symbols and no chunk is longer than 65,535; otherwise, and in
 * the device-resident _var calls (whose chunk lengths the host does not see), as u32 in a workspace
 * the context owns (cnt=global), which calls on one context therefore must not share between
 * streams running at the same time. */
int ans_gpu_mset_pop_slack(uint64_t chunk_len, uint64_t *bytes);
int ans_dev_mset_push(ans_gpu_tableset *ts, uint32_t table, const void *d_syms, int sym_bytes, uint64_t n,
                      uint64_t chunk_len, uint8_t *d_slots, uint64_t slot_cap, uint32_t *d_lens /* in/out */,
                      uint32_t *d_status, void *stream);
int ans_dev_mset_pop(ans_gpu_tableset *ts, uint32_t table, uint8_t *d_slots /* in/out */, uint64_t slot_cap,
                     uint32_t *d_lens /* in/out */, uint64_t n, uint64_t chunk_len, void *d_syms, int sym_bytes,
                     uint32_t *d_status, void *stream);
int ans_dev_mset_push_var(ans_gpu_tableset *ts, uint32_t table, const void *d_syms, int sym_bytes, uint64_t nchunks,
                          const uint64_t *d_starts, uint8_t *d_slots, uint64_t slot_cap,
                          uint32_t *d_lens /* in/out */, uint32_t *d_status, void *stream);
int ans_dev_mset_pop_var(ans_gpu_tableset *ts, uint32_t table, uint8_t *d_slots /* in/out */, uint64_t slot_cap,
                         uint32_t *d_lens /* in/out */, uint64_t nchunks, const uint64_t *d_starts, void *d_syms,
                         int sym_bytes, uint32_t *d_status, void *stream);
/* ... on host buffers, synchronous, a dense container in and one out exactly as the
 * ans_gpu_independent_push_chunks family (out == NULL is the size query; pop still fills out_syms). */
int ans_gpu_mset_push_chunks(ans_gpu_tableset *ts, uint32_t table, const void *syms, int sym_bytes, uint64_t n,
                             uint64_t chunk_len, const uint8_t *in, uint64_t in_len, const uint64_t *in_offsets,
                             const uint64_t *in_lens, uint8_t *out, uint64_t out_cap, uint64_t *offsets,
                             uint64_t *lens, uint64_t *total);
int ans_gpu_mset_pop_chunks(ans_gpu_tableset *ts, uint32_t table, const uint8_t *in, uint64_t in_len,
                            const uint64_t *in_offsets, const uint64_t *in_lens, uint64_t n, uint64_t chunk_len,
                            void *out_syms, int sym_bytes, uint8_t *out, uint64_t out_cap, uint64_t *offsets,
                            uint64_t *lens, uint64_t *total);
int ans_gpu_mset_push_var_chunks(ans_gpu_tableset *ts, uint32_t table, const void *syms, int sym_bytes,
                                 uint64_t nchunks, const uint64_t *starts, const uint8_t *in, uint64_t in_len,
                                 const uint64_t *in_offsets, const uint64_t *in_lens, uint8_t *out, uint64_t out_cap,
                                 uint64_t *offsets, uint64_t *lens, uint64_t *total);
int ans_gpu_mset_pop_var_chunks(ans_gpu_tableset *ts, uint32_t table, const uint8_t *in, uint64_t in_len,
                                const uint64_t *in_offsets, const uint64_t *in_lens, uint64_t nchunks,
                                const uint64_t *starts, void *out_syms, int sym_bytes, uint8_t *out, uint64_t out_cap,
                                uint64_t *offsets, uint64_t *lens, uint64_t *total);

/* ======================================================================
 * (5) Graph models' bulk-IID caller — DenseSetIID<EdgeIndex, AllEdgeIndices> with an
 *     IID<Bernoulli> (ErdosRenyi, src/graph_codec.rs:105-205).  Edges are uint32 pairs
 *     (i, j) (EdgeIndex, src/graph.rs:17), num_nodes < 2^32.  The alphabet is the reference's
 *     AllEdgeIndices order (src/graph_codec.rs:187-199): self-loops (i,i) first when `loops`,
 *     then for j in 0..n, i in 0..j: (i,j), followed by (j,i) when `directed`.  An edge outside
 *     the alphabet (undirected (j,i) with j > i, a loop without `loops`, a node >= n) is
 *     ANS_E_SYMBOL, where DenseSetIID::dense panics (src/graph_codec.rs:137).
 * ====================================================================== */
/* num_all_edge_indices  src/graph_codec.rs:203-205 */
int ans_edge_alphabet_len(uint64_t num_nodes, int directed, int loops, uint64_t *len);
/* DenseSetIID::dense  src/graph_codec.rs:133-138: d_dense[slot(edge)] = 1, others 0 (u8) */
int ans_dev_edges_to_dense(ans_gpu *g, uint64_t num_nodes, int directed, int loops, const uint32_t *d_edges,
                           uint64_t num_edges, uint8_t *d_dense, uint32_t *d_status, void *stream);
/* the filter of DenseSetIID::pop  src/graph_codec.rs:117-120: the set slots' edges in
 * alphabet order into d_edges (at most cap; ANS_E_LEN in *d_status beyond), count in *d_count */
int ans_dev_dense_to_edges(ans_gpu *g, uint64_t num_nodes, int directed, int loops, const uint8_t *d_dense,
                           uint32_t *d_edges, uint64_t cap, uint64_t *d_count, uint32_t *d_status, void *stream);
/* ErdosRenyi push / pop (src/graph_codec.rs:152-155), chunked like section (4): the dense
 * vector over the alphabet, coded with a Bernoulli table (ans_table_create_bernoulli; the
 * reference's Bernoulli::new(total_edges, total_possible_edges), src/benchmark.rs:556);
 * chunk j is one reference message over slots [j*chunk_len, (j+1)*chunk_len). */
int ans_gpu_dense_set_encode(ans_gpu_table *gt, uint64_t num_nodes, int directed, int loops, const uint32_t *edges,
                             uint64_t num_edges, uint64_t chunk_len, uint8_t *out, uint64_t out_cap,
                             uint64_t *offsets, uint64_t *lens, uint64_t *total);
int ans_gpu_dense_set_decode(ans_gpu_table *gt, uint64_t num_nodes, int directed, int loops, const uint8_t *in,
                             uint64_t in_len, const uint64_t *offsets, const uint64_t *lens, uint64_t chunk_len,
                             uint32_t *edges, uint64_t cap, uint64_t *num_edges);

/* Independent<GraphIID<ErdosRenyi>> over a dataset of graphs (GraphDatasetParamCodec with
 * ErdosRenyiParamCodec: one Bernoulli gt for every graph, src/param_codec.rs:171-199,243-293).
 * Graph g has num_nodes[g] nodes and the edges [edge_offsets[g], edge_offsets[g+1]) of `edges`
 * (uint32 pairs).  Graph g is chunk g of the variable-chunk path: its stream is the reference
 * message Message::zeros() + ErdosRenyi push of that graph alone.  Decode returns every graph's
 * edges in alphabet order, graph after graph, with edge_offsets (num_graphs + 1 entries) giving
 * each graph's range; ANS_E_LEN when they exceed cap (edge_offsets still complete). */
int ans_gpu_dense_sets_encode(ans_gpu_table *gt, uint64_t num_graphs, const uint32_t *num_nodes, int directed,
                              int loops, const uint32_t *edges, const uint64_t *edge_offsets, uint8_t *out,
                              uint64_t out_cap, uint64_t *offsets, uint64_t *lens, uint64_t *total);
int ans_gpu_dense_sets_decode(ans_gpu_table *gt, uint64_t num_graphs, const uint32_t *num_nodes, int directed,
                              int loops, const uint8_t *in, uint64_t in_len, const uint64_t *offsets,
                              const uint64_t *lens, uint32_t *edges, uint64_t cap, uint64_t *edge_offsets);

/* ======================================================================
 * (5b) GraphIID<NodeC, EdgeC, ErdosRenyi> over a dataset (src/graph_codec.rs:19-94), the model
 *      the reference's --er runs on node- and edge-labelled datasets: Independent of one
 *      GraphIID per graph (src/benchmark.rs:308-316, 349-358) with count-built Categorical labels
 *      (DatasetStats::node_label_dist / edge_label_dist, src/benchmark.rs:568-578) or, for
 *      --uniform-er, Uniform(size) labels (src/benchmark.rs:318-330, 360-372: pass the all-ones
 *      Categorical of that size, whose arithmetic is Uniform's: pmf 1, cdf x, norm size).
 *      Tables come from one table set: node_table and edge_table index it (ANS_NO_TABLE =
 *      EmptyCodec, nothing coded), edge_indicator_table is the Bernoulli (two symbols).  Graph g
 *      (num_nodes[g] nodes, node labels [sum of earlier num_nodes, + num_nodes[g]) of node_labels,
 *      edges [edge_offsets[g], edge_offsets[g+1]) of edges / edge_labels) is ONE message:
 *      Message::zeros() (or gen_kind / seed as in the _ex calls, graph g from seed + g), then
 *      GraphIID::push, i.e. EdgesIID::push (the edge labels sorted by edge index as a tuple
 *      (i, j), then the ErdosRenyi indicator vector) followed by IID<NodeC>::push of the node
 *      labels (src/graph_codec.rs:31-34, 61-65); its stream is that message flattened.
 *      Edges are uint32 pairs in the alphabet of section 5 (undirected: i <= j); an edge outside
 *      it, or with labelled edges a pair given twice, is ANS_E_SYMBOL; a label outside its table
 *      is ANS_E_SYMBOL.  Required lengths, which the library cannot check and reads in full:
 *      with a node table, node_labels holds sum(num_nodes) entries (num_nodes[g] per graph, no
 *      gaps); with an edge table, edge_labels holds edge_offsets[num_graphs] entries, entry k the
 *      label of edge k (one per edge of every graph); edges holds 2 * edge_offsets[num_graphs]
 *      entries.  A shorter buffer is read past its end.  Decode pops node labels, the indicator vector, then as many edge labels
 *      as the vector holds edges (src/graph_codec.rs:36-38, 67-71) and returns every graph's
 *      edges sorted by (i, j) -- EdgesIID::pop's `indices.sort_unstable()` -- with their labels
 *      beside them, graph after graph; edge_offsets (num_graphs + 1) gives each graph's range;
 *      ANS_E_LEN when the edges exceed cap (edge_offsets still complete).
 * ====================================================================== */
#define ANS_NO_TABLE 0xFFFFFFFFu
int ans_gpu_graphs_encode(ans_gpu_tableset *ts, uint32_t node_table, uint32_t edge_table,
                          uint32_t edge_indicator_table, int directed, int loops, uint64_t num_graphs,
                          const uint32_t *num_nodes, const uint32_t *node_labels, const uint32_t *edges,
                          const uint32_t *edge_labels, const uint64_t *edge_offsets, int gen_kind, uint64_t seed,
                          uint8_t *out, uint64_t out_cap, uint64_t *offsets, uint64_t *lens, uint64_t *total);
int ans_gpu_graphs_decode(ans_gpu_tableset *ts, uint32_t node_table, uint32_t edge_table,
                          uint32_t edge_indicator_table, int directed, int loops, uint64_t num_graphs,
                          const uint32_t *num_nodes, const uint8_t *in, uint64_t in_len, const uint64_t *offsets,
                          const uint64_t *lens, int gen_kind, uint64_t seed, uint32_t *node_labels, uint32_t *edges,
                          uint32_t *edge_labels, uint64_t cap, uint64_t *edge_offsets);

/* ======================================================================
 * (5c) The Pólya urn edge-index codec in bulk: ans_polya_push / ans_polya_pop (section 3) of graph
 *      g's edges onto / from the message ALREADY in slot g, one lane per graph, under the resume
 *      contract of section 4b word for word: the input is Message::unflatten(slot bytes, d_lens[g])
 *      with the Empty tail, the result is flattened back into the slot and d_lens[g] is its length
 *      (a graph without edges grows by the one 0x00 of flatten).  The bytes equal the host codec's.
 *      Graph g has d_num_nodes[g] nodes and the pairs [d_edge_offsets[g], d_edge_offsets[g+1]) of
 *      d_edges (num_graphs + 1 offsets; pop WRITES the pairs there: the caller supplies the offsets,
 *      E being a parameter of the model).  With push after ans_dev_independent_push_var of the edge
 *      labels and before that of the node labels, slot g holds GraphIID<NodeC, EdgeC, PolyaUrn>.
 *      Statuses are OR-ed into *d_status with d_lens[g] = 0 for that graph alone: those of
 *      ans_polya_push / _pop; ANS_E_ARG for a graph of more than max_nodes nodes or max_edges edges;
 *      ANS_E_LEN for a result past slot_cap or a d_lens[g] above it.  With slot_cap >= d_lens[g] +
 *      ans_gpu_polya_slack(max_nodes, max_edges) neither call meets ANS_E_LEN: the slack is
 *      (max_edges / 8 + 1) * max(2 bitlen(max_nodes + 2 max_edges), bitlen(max_edges) + 1)
 *      + max_edges / 2^20 + 16 bytes (a push adds two urn symbols per edge, a pop puts an orbit
 *      and an orientation bit back).  The host-buffer calls apply it themselves.
 *      The per-lane state (2 max_nodes + 6 max_edges + 2 dwords) lives in the workspace the
 *      multiset kernels' cnt=global form uses, which calls on one context therefore must not share
 *      between streams running at the same time; it is sized by the lanes resident, at most
 *      256 MiB, and max_nodes / max_edges whose single wave passes that are ANS_E_ARG, as are
 *      max_edges >= 2^31.  Kernel names in ans_gpu_last_launch: k_polya_push<redraws=0>,
 *      k_polya_pop<redraws=1>.
 * ====================================================================== */
int ans_gpu_polya_slack(uint32_t max_nodes, uint64_t max_edges, uint64_t *bytes);
int ans_dev_polya_push(ans_gpu *g, int loops, int redraws, uint64_t num_graphs, const uint32_t *d_num_nodes,
                       const uint32_t *d_edges, const uint64_t *d_edge_offsets, uint32_t max_nodes,
                       uint64_t max_edges, uint8_t *d_slots, uint64_t slot_cap, uint32_t *d_lens /* in/out */,
                       uint32_t *d_status, void *stream);
int ans_dev_polya_pop(ans_gpu *g, int loops, int redraws, uint64_t num_graphs, const uint32_t *d_num_nodes,
                      uint32_t *d_edges /* out */, const uint64_t *d_edge_offsets, uint32_t max_nodes,
                      uint64_t max_edges, uint8_t *d_slots /* in/out */, uint64_t slot_cap,
                      uint32_t *d_lens /* in/out */, uint32_t *d_status, void *stream);
/* ... on host buffers, synchronous, a dense container in and one out exactly as
 * ans_gpu_mset_push_var_chunks / _pop_var_chunks (out == NULL is the size query; pop still fills
 * out_edges, edge_offsets[num_graphs] pairs). */
int ans_gpu_polya_push_graphs(ans_gpu *g, int loops, int redraws, uint64_t num_graphs, const uint32_t *num_nodes,
                              const uint32_t *edges, const uint64_t *edge_offsets, const uint8_t *in, uint64_t in_len,
                              const uint64_t *in_offsets, const uint64_t *in_lens, uint8_t *out, uint64_t out_cap,
                              uint64_t *offsets, uint64_t *lens, uint64_t *total);
int ans_gpu_polya_pop_graphs(ans_gpu *g, int loops, int redraws, uint64_t num_graphs, const uint32_t *num_nodes,
                             const uint64_t *edge_offsets, const uint8_t *in, uint64_t in_len,
                             const uint64_t *in_offsets, const uint64_t *in_lens, uint32_t *out_edges, uint8_t *out,
                             uint64_t out_cap, uint64_t *offsets, uint64_t *lens, uint64_t *total);

/* ======================================================================
 * (5d) The autoregressive Erdős–Rényi graph codecs in bulk: ans_ar_er_push / ans_ar_er_pop
 *      (section 3) of graph g onto / from the message ALREADY in slot g, one lane per graph, under
 *      the resume contract of section 4b as section 5c has it: the input is Message::unflatten(slot
 *      bytes, d_lens[g]) with the Empty tail, the result is flattened back into the slot and
 *      d_lens[g] is its length.  The bytes equal the host codec's.  gt is the Bernoulli (two symbols,
 *      else ANS_E_ARG; any norm a table takes).
 *      push: graph g has d_num_nodes[g] nodes and the pairs [d_edge_offsets[g], d_edge_offsets[g+1])
 *      of d_edges (num_graphs + 1 offsets); d_perm is NULL or holds num_graphs * max_nodes entries,
 *      graph g's permutation at d_perm + g * max_nodes.
 *      pop: the offsets are CAPACITIES: graph g's pairs are written from d_edge_offsets[g] on, at most
 *      d_edge_offsets[g+1] - d_edge_offsets[g] of them, and d_num_edges[g] is their number.
 *      Statuses are OR-ed into *d_status with d_lens[g] = 0 (and d_num_edges[g] = 0) for that graph
 *      alone: those of ans_ar_er_push / _pop; ANS_E_ARG for a graph of more than max_nodes nodes or
 *      (push) max_edges pairs; ANS_E_LEN for a result past slot_cap, a d_lens[g] above it, or more
 *      pairs than the graph's capacity.  With slot_cap >= d_lens[g] + ans_gpu_ar_er_slack(gt,
 *      max_nodes, loops) neither call meets ANS_E_LEN for a slot: with s = max_nodes (max_nodes - 1)
 *      / 2 + max_nodes * loops indicators, pmin the smaller nonzero mass, the slack is
 *      max(s * (bitlen(norm / pmin) + (norm > 2^36)), max_nodes * bitlen(max_nodes)) / 8 + 1
 *      + (s + max_nodes) / 2^20 + 16 bytes.  The host-buffer calls apply it.
 *      The per-lane state (push: 6 max_nodes + 2 max_edges + 2 dwords, pop: 2 max_nodes + 1) lives in
 *      the workspace of sections 4b / 5c, under the same rule: calls on one context must not share
 *      it between streams running at the same time; it is sized by the lanes resident, at most
 *      256 MiB, and bounds whose single wave passes that are ANS_E_ARG before anything is launched,
 *      as are max_edges >= 2^31.  The degrees' class ranks are a table of max_nodes + 1 entries the
 *      context keeps; a call with another max_nodes rebuilds it, which waits for the device.
 *      Kernel names in ans_gpu_last_launch: k_arer_push<orbits=2>, k_arer_pop<orbits=0>, their
 *      workgroups in ans_gpu_last_launch_grid.
 * ====================================================================== */
int ans_gpu_ar_er_slack(const ans_gpu_table *gt, uint32_t max_nodes, int loops, uint64_t *bytes);
int ans_dev_ar_er_push(ans_gpu_table *gt, int loops, int orbits, uint64_t num_graphs, const uint32_t *d_num_nodes,
                       const uint32_t *d_edges, const uint64_t *d_edge_offsets, uint32_t max_nodes,
                       uint64_t max_edges, uint32_t *d_perm /* NULL or num_graphs * max_nodes */, uint8_t *d_slots,
                       uint64_t slot_cap, uint32_t *d_lens /* in/out */, uint32_t *d_status, void *stream);
int ans_dev_ar_er_pop(ans_gpu_table *gt, int loops, int orbits, uint64_t num_graphs, const uint32_t *d_num_nodes,
                      uint32_t *d_edges /* out */, const uint64_t *d_edge_offsets /* capacities */,
                      uint32_t *d_num_edges /* out */, uint32_t max_nodes, uint8_t *d_slots /* in/out */,
                      uint64_t slot_cap, uint32_t *d_lens /* in/out */, uint32_t *d_status, void *stream);
/* ... on host buffers, synchronous, a dense container in and one out exactly as
 * ans_gpu_polya_push_graphs / _pop_graphs (out == NULL is the size query; pop still fills out_edges
 * and out_num_edges).  perm is NULL or holds num_graphs * (the largest num_nodes) entries, graph g's
 * at perm + g * that.  pop: edge_offsets are capacities as above, out_num_edges[g] the pairs of graph g. */
int ans_gpu_ar_er_push_graphs(ans_gpu_table *gt, int loops, int orbits, uint64_t num_graphs, const uint32_t *num_nodes,
                              const uint32_t *edges, const uint64_t *edge_offsets, const uint8_t *in, uint64_t in_len,
                              const uint64_t *in_offsets, const uint64_t *in_lens, uint32_t *perm, uint8_t *out,
                              uint64_t out_cap, uint64_t *offsets, uint64_t *lens, uint64_t *total);
int ans_gpu_ar_er_pop_graphs(ans_gpu_table *gt, int loops, int orbits, uint64_t num_graphs, const uint32_t *num_nodes,
                             const uint64_t *edge_offsets, const uint8_t *in, uint64_t in_len,
                             const uint64_t *in_offsets, const uint64_t *in_lens, uint32_t *out_edges,
                             uint32_t *out_num_edges, uint8_t *out, uint64_t out_cap, uint64_t *offsets,
                             uint64_t *lens, uint64_t *total);

/* ======================================================================
 * (5e) The autoregressive Pólya urn graph codecs in bulk: ans_ar_polya_push / ans_ar_polya_pop
 *      (section 3) of graph g onto / from the message ALREADY in slot g, one lane per graph, under
 *      the resume contract exactly as section 5d has it (slots, d_lens, d_perm, the offsets as
 *      CAPACITIES on a pop, d_num_edges, the statuses OR-ed into *d_status with d_lens[g] = 0 for the
 *      failing graph alone).  The bytes equal the host codec's.  The model has no parameters, so the
 *      calls take the context where section 5d takes the table.
 *      ANS_E_ARG for a graph of more than max_nodes nodes or (push) max_edges pairs; ANS_E_LEN for a
 *      result past slot_cap, a d_lens[g] above it, or more pairs than the graph's capacity.  With
 *      slot_cap >= d_lens[g] + ans_gpu_ar_polya_slack(max_nodes, max_edges) neither call meets
 *      ANS_E_LEN for a slot (pop: max_edges bounds the pairs a graph can hold, its capacity at most):
 *      with bn = bitlen(max_nodes) the slack is
 *        max(max_nodes * (bitlen(bn + 2) + bn) + max_edges * bitlen(max_nodes + max_edges),
 *            (max_nodes + max_edges) * bn) / 8 + 1 + (2 max_nodes + 2 max_edges) / 2^20 + 16 bytes
 *      (DESIGN.md section 3.11).  The host-buffer calls apply it.
 *      The per-lane state (push: 13 max_nodes + 2 max_edges + 2 dwords, pop: 9 max_nodes + min(max_nodes, 11) + 1) lives
 *      in the workspace of sections 4b / 5c / 5d under the same rule, at most 256 MiB; bounds whose
 *      single wave passes that are ANS_E_ARG before anything is launched or recorded, as are
 *      max_edges >= 2^31.  The degrees' class ranks are the table of section 5d.
 *      Kernel names in ans_gpu_last_launch: k_arpu_push<orbits=2>, k_arpu_pop<orbits=0>, their
 *      workgroups in ans_gpu_last_launch_grid.
 * ====================================================================== */
int ans_gpu_ar_polya_slack(uint32_t max_nodes, uint64_t max_edges, uint64_t *bytes);
int ans_dev_ar_polya_push(ans_gpu *g, int loops, int orbits, uint64_t num_graphs, const uint32_t *d_num_nodes,
                          const uint32_t *d_edges, const uint64_t *d_edge_offsets, uint32_t max_nodes,
                          uint64_t max_edges, uint32_t *d_perm /* NULL or num_graphs * max_nodes */,
                          uint8_t *d_slots, uint64_t slot_cap, uint32_t *d_lens /* in/out */, uint32_t *d_status,
                          void *stream);
int ans_dev_ar_polya_pop(ans_gpu *g, int loops, int orbits, uint64_t num_graphs, const uint32_t *d_num_nodes,
                         uint32_t *d_edges /* out */, const uint64_t *d_edge_offsets /* capacities */,
                         uint32_t *d_num_edges /* out */, uint32_t max_nodes, uint64_t max_edges /* the slack's */,
                         uint8_t *d_slots /* in/out */, uint64_t slot_cap, uint32_t *d_lens /* in/out */,
                         uint32_t *d_status, void *stream);
/* ... on host buffers, synchronous, exactly as ans_gpu_ar_er_push_graphs / _pop_graphs. */
int ans_gpu_ar_polya_push_graphs(ans_gpu *g, int loops, int orbits, uint64_t num_graphs, const uint32_t *num_nodes,
                                 const uint32_t *edges, const uint64_t *edge_offsets, const uint8_t *in,
                                 uint64_t in_len, const uint64_t *in_offsets, const uint64_t *in_lens, uint32_t *perm,
                                 uint8_t *out, uint64_t out_cap, uint64_t *offsets, uint64_t *lens, uint64_t *total);
int ans_gpu_ar_polya_pop_graphs(ans_gpu *g, int loops, int orbits, uint64_t num_graphs, const uint32_t *num_nodes,
                                const uint64_t *edge_offsets, const uint8_t *in, uint64_t in_len,
                                const uint64_t *in_offsets, const uint64_t *in_lens, uint32_t *out_edges,
                                uint32_t *out_num_edges, uint8_t *out, uint64_t out_cap, uint64_t *offsets,
                                uint64_t *lens, uint64_t *total);

/* ======================================================================
 * (5f) The same codecs with Weisfeiler-Lehman orbits in bulk: ans_ar_er_wl_push / _pop and
 *      ans_ar_polya_wl_push / _pop (section 3) of graph g onto / from the message ALREADY in slot g,
 *      one lane per graph, under the resume contract exactly as sections 5d / 5e have it (slots,
 *      d_lens, d_perm, the offsets as CAPACITIES on a pop, d_num_edges, the statuses OR-ed into
 *      *d_status with d_lens[g] = 0 for the failing graph alone).  The bytes equal the host codec's.
 *      wl_iter above ANS_WL_MAX_ITER is ANS_E_ARG.  A pop keeps the decoded prefix's adjacency, so
 *      both pops take max_edges and hold min(capacity, max_edges) pairs of a graph; one more is
 *      ANS_E_LEN for that graph.
 *      Slack: an orbit step still pops under the norm L <= max_nodes on a push and pushes at most
 *      bitlen(max_nodes) bits per node on a pop, whatever the classes are, so the derivations of
 *      ans_gpu_ar_er_slack and ans_gpu_ar_polya_slack hold unchanged: with slot_cap >= d_lens[g] +
 *      that slack neither call meets ANS_E_LEN for a slot.  The host-buffer calls apply it.
 *      The per-lane state, with K = wl_iter + 1 and o = (2K + 4 + 2 (wl_iter > 0)) max_nodes dwords
 *      of orbit stage (the ids, the ordered known positions and their inverse, the dirty list and
 *      its stamps, the sort scratch): Erdős–Rényi push 4 max_nodes + 2 max_edges + 1 + o, pop
 *      2 max_nodes + 2 max_edges + o; Pólya urn push 11 max_nodes + 2 max_edges + 1 + o, pop
 *      9 max_nodes + min(max_nodes, 11) + 2 max_edges + o.  It lives in the workspace of sections
 *      4b / 5c / 5d under the same rule, at most 256 MiB; bounds whose single wave passes that are
 *      ANS_E_ARG before anything is launched or recorded, as are max_edges >= 2^31.
 *      Kernel names in ans_gpu_last_launch: k_arer_wl_push(wl_iter=1,half_iter=1), k_arer_wl_pop(..),
 *      k_arpu_wl_push(..), k_arpu_wl_pop(..), their workgroups in ans_gpu_last_launch_grid.
 * ====================================================================== */
int ans_dev_ar_er_wl_push(ans_gpu_table *gt, int loops, int wl_iter, int half_iter, uint64_t num_graphs,
                          const uint32_t *d_num_nodes, const uint32_t *d_edges, const uint64_t *d_edge_offsets,
                          uint32_t max_nodes, uint64_t max_edges, uint32_t *d_perm /* NULL or num_graphs * max_nodes */,
                          uint8_t *d_slots, uint64_t slot_cap, uint32_t *d_lens /* in/out */, uint32_t *d_status,
                          void *stream);
int ans_dev_ar_er_wl_pop(ans_gpu_table *gt, int loops, int wl_iter, int half_iter, uint64_t num_graphs,
                         const uint32_t *d_num_nodes, uint32_t *d_edges /* out */,
                         const uint64_t *d_edge_offsets /* capacities */, uint32_t *d_num_edges /* out */,
                         uint32_t max_nodes, uint64_t max_edges, uint8_t *d_slots /* in/out */, uint64_t slot_cap,
                         uint32_t *d_lens /* in/out */, uint32_t *d_status, void *stream);
int ans_dev_ar_polya_wl_push(ans_gpu *g, int loops, int wl_iter, int half_iter, uint64_t num_graphs,
                             const uint32_t *d_num_nodes, const uint32_t *d_edges, const uint64_t *d_edge_offsets,
                             uint32_t max_nodes, uint64_t max_edges, uint32_t *d_perm, uint8_t *d_slots,
                             uint64_t slot_cap, uint32_t *d_lens /* in/out */, uint32_t *d_status, void *stream);
int ans_dev_ar_polya_wl_pop(ans_gpu *g, int loops, int wl_iter, int half_iter, uint64_t num_graphs,
                            const uint32_t *d_num_nodes, uint32_t *d_edges /* out */,
                            const uint64_t *d_edge_offsets /* capacities */, uint32_t *d_num_edges /* out */,
                            uint32_t max_nodes, uint64_t max_edges, uint8_t *d_slots /* in/out */, uint64_t slot_cap,
                            uint32_t *d_lens /* in/out */, uint32_t *d_status, void *stream);
/* ... on host buffers, synchronous, exactly as ans_gpu_ar_er_push_graphs / _pop_graphs. */
int ans_gpu_ar_er_wl_push_graphs(ans_gpu_table *gt, int loops, int wl_iter, int half_iter, uint64_t num_graphs,
                                 const uint32_t *num_nodes, const uint32_t *edges, const uint64_t *edge_offsets,
                                 const uint8_t *in, uint64_t in_len, const uint64_t *in_offsets,
                                 const uint64_t *in_lens, uint32_t *perm, uint8_t *out, uint64_t out_cap,
                                 uint64_t *offsets, uint64_t *lens, uint64_t *total);
int ans_gpu_ar_er_wl_pop_graphs(ans_gpu_table *gt, int loops, int wl_iter, int half_iter, uint64_t num_graphs,
                                const uint32_t *num_nodes, const uint64_t *edge_offsets, const uint8_t *in,
                                uint64_t in_len, const uint64_t *in_offsets, const uint64_t *in_lens,
                                uint32_t *out_edges, uint32_t *out_num_edges, uint8_t *out, uint64_t out_cap,
                                uint64_t *offsets, uint64_t *lens, uint64_t *total);
int ans_gpu_ar_polya_wl_push_graphs(ans_gpu *g, int loops, int wl_iter, int half_iter, uint64_t num_graphs,
                                    const uint32_t *num_nodes, const uint32_t *edges, const uint64_t *edge_offsets,
                                    const uint8_t *in, uint64_t in_len, const uint64_t *in_offsets,
                                    const uint64_t *in_lens, uint32_t *perm, uint8_t *out, uint64_t out_cap,
                                    uint64_t *offsets, uint64_t *lens, uint64_t *total);
int ans_gpu_ar_polya_wl_pop_graphs(ans_gpu *g, int loops, int wl_iter, int half_iter, uint64_t num_graphs,
                                   const uint32_t *num_nodes, const uint64_t *edge_offsets, const uint8_t *in,
                                   uint64_t in_len, const uint64_t *in_offsets, const uint64_t *in_lens,
                                   uint32_t *out_edges, uint32_t *out_num_edges, uint8_t *out, uint64_t out_cap,
                                   uint64_t *offsets, uint64_t *lens, uint64_t *total);

/* ======================================================================
 * (5g) The same codecs for graphs with node and edge labels in bulk: ans_ar_er_wl_labelled_push /
 *      _pop and ans_ar_polya_wl_labelled_push / _pop (section 3) of graph g onto / from the message
 *      ALREADY in slot g, one lane per graph, under the resume contract exactly as section 5f has it.
 *      The bytes equal the host codec's.  Tables come from one table set, as ans_gpu_graphs_encode
 *      has them: bern_table (two symbols: the Erdős–Rényi indicator; the Pólya urn calls take none),
 *      node_table and edge_table index it, ANS_NO_TABLE = no such label (EmptyCodec).  A label table
 *      needs its array and an array its table, else ANS_E_ARG.  With both ANS_NO_TABLE the slots,
 *      lens and perm are those of section 5f; a pop's pairs differ only in that a node's loop comes
 *      first under the Erdős–Rényi slices too.
 *        d_node_labels  num_graphs x max_nodes, graph g's labels at g * max_nodes (as d_perm): by input
 *                       node on a push, by position on a pop;
 *        d_edge_labels  one entry per pair, at the pairs' offsets: entry d_edge_offsets[g] + k is the
 *                       label of graph g's pair k.
 *      Statuses per graph as 5f, and ANS_E_SYMBOL for a label outside its table, ANS_E_ZERO_MASS for
 *      one of mass 0 (the slot's message is then dropped as for every failing graph: d_lens[g] = 0).
 *      Slack: ans_gpu_ar_er_wl_labelled_slack / ans_gpu_ar_polya_wl_labelled_slack add to the slack of
 *      5d / 5e the bytes max_nodes node-label pushes and max_edges edge-label pushes can add: a push
 *      under a table of norm N and smallest non-zero mass pmin adds fewer than bitlen(N / pmin) bits,
 *      one more when N > 2^36; a pop takes labels off and adds none.  With
 *      slot_cap >= d_lens[g] + that slack neither call meets ANS_E_LEN for a slot; the host-buffer
 *      calls apply it.
 *      The per-lane state is 5f's with, under an edge table, o grown by max_nodes dwords at wl_iter > 0
 *      (the sort scratch holds (hash, label) keys of three dwords) and by 2 max_nodes at wl_iter = 0
 *      (the labels the half iteration sorts), and on a push 2 max_edges + 2 max_nodes dwords more (the
 *      label of each adjacency entry, the slice's positions and labels).  A node table adds nothing.
 *      The same 256 MiB rule holds: bounds whose single wave passes it are ANS_E_ARG before anything is
 *      launched or recorded.  The table set's image is staged in LDS when it is at most 48 KiB.
 *      Kernel names in ans_gpu_last_launch: k_arer_wll_push(wl_iter=1,half_iter=1,node=1,edge=1),
 *      k_arer_wll_pop(..), k_arpu_wll_push(..), k_arpu_wll_pop(..).
 * ====================================================================== */
int ans_gpu_ar_er_wl_labelled_slack(const ans_gpu_tableset *ts, uint32_t bern_table, uint32_t node_table,
                                    uint32_t edge_table, uint32_t max_nodes, uint64_t max_edges, int loops,
                                    uint64_t *bytes);
int ans_gpu_ar_polya_wl_labelled_slack(const ans_gpu_tableset *ts, uint32_t node_table, uint32_t edge_table,
                                       uint32_t max_nodes, uint64_t max_edges, uint64_t *bytes);
int ans_dev_ar_er_wl_labelled_push(ans_gpu_tableset *ts, uint32_t bern_table, uint32_t node_table, uint32_t edge_table,
                                   int loops, int wl_iter, int half_iter, uint64_t num_graphs,
                                   const uint32_t *d_num_nodes, const uint32_t *d_edges, const uint64_t *d_edge_offsets,
                                   const uint32_t *d_node_labels, const uint32_t *d_edge_labels, uint32_t max_nodes,
                                   uint64_t max_edges, uint32_t *d_perm /* NULL or num_graphs * max_nodes */,
                                   uint8_t *d_slots, uint64_t slot_cap, uint32_t *d_lens /* in/out */,
                                   uint32_t *d_status, void *stream);
int ans_dev_ar_er_wl_labelled_pop(ans_gpu_tableset *ts, uint32_t bern_table, uint32_t node_table, uint32_t edge_table,
                                  int loops, int wl_iter, int half_iter, uint64_t num_graphs,
                                  const uint32_t *d_num_nodes, uint32_t *d_edges /* out */,
                                  const uint64_t *d_edge_offsets /* capacities */, uint32_t *d_num_edges /* out */,
                                  uint32_t *d_node_labels /* out */, uint32_t *d_edge_labels /* out */,
                                  uint32_t max_nodes, uint64_t max_edges, uint8_t *d_slots /* in/out */,
                                  uint64_t slot_cap, uint32_t *d_lens /* in/out */, uint32_t *d_status, void *stream);
int ans_dev_ar_polya_wl_labelled_push(ans_gpu_tableset *ts, uint32_t node_table, uint32_t edge_table, int loops,
                                      int wl_iter, int half_iter, uint64_t num_graphs, const uint32_t *d_num_nodes,
                                      const uint32_t *d_edges, const uint64_t *d_edge_offsets,
                                      const uint32_t *d_node_labels, const uint32_t *d_edge_labels, uint32_t max_nodes,
                                      uint64_t max_edges, uint32_t *d_perm, uint8_t *d_slots, uint64_t slot_cap,
                                      uint32_t *d_lens /* in/out */, uint32_t *d_status, void *stream);
int ans_dev_ar_polya_wl_labelled_pop(ans_gpu_tableset *ts, uint32_t node_table, uint32_t edge_table, int loops,
                                     int wl_iter, int half_iter, uint64_t num_graphs, const uint32_t *d_num_nodes,
                                     uint32_t *d_edges /* out */, const uint64_t *d_edge_offsets /* capacities */,
                                     uint32_t *d_num_edges /* out */, uint32_t *d_node_labels /* out */,
                                     uint32_t *d_edge_labels /* out */, uint32_t max_nodes, uint64_t max_edges,
                                     uint8_t *d_slots /* in/out */, uint64_t slot_cap, uint32_t *d_lens /* in/out */,
                                     uint32_t *d_status, void *stream);
/* ... on host buffers, synchronous, exactly as ans_gpu_ar_er_wl_push_graphs / _pop_graphs; node_labels
 * is num_graphs x the largest num_nodes, graph g's labels at g times that (as perm), edge_labels holds
 * one entry per pair of edges (a pop: per capacity). */
int ans_gpu_ar_er_wl_labelled_push_graphs(ans_gpu_tableset *ts, uint32_t bern_table, uint32_t node_table,
                                          uint32_t edge_table, int loops, int wl_iter, int half_iter,
                                          uint64_t num_graphs, const uint32_t *num_nodes, const uint32_t *edges,
                                          const uint64_t *edge_offsets, const uint32_t *node_labels,
                                          const uint32_t *edge_labels, const uint8_t *in, uint64_t in_len,
                                          const uint64_t *in_offsets, const uint64_t *in_lens, uint32_t *perm,
                                          uint8_t *out, uint64_t out_cap, uint64_t *offsets, uint64_t *lens,
                                          uint64_t *total);
int ans_gpu_ar_er_wl_labelled_pop_graphs(ans_gpu_tableset *ts, uint32_t bern_table, uint32_t node_table,
                                         uint32_t edge_table, int loops, int wl_iter, int half_iter,
                                         uint64_t num_graphs, const uint32_t *num_nodes, const uint64_t *edge_offsets,
                                         const uint8_t *in, uint64_t in_len, const uint64_t *in_offsets,
                                         const uint64_t *in_lens, uint32_t *out_edges, uint32_t *out_num_edges,
                                         uint32_t *out_node_labels, uint32_t *out_edge_labels, uint8_t *out,
                                         uint64_t out_cap, uint64_t *offsets, uint64_t *lens, uint64_t *total);
int ans_gpu_ar_polya_wl_labelled_push_graphs(ans_gpu_tableset *ts, uint32_t node_table, uint32_t edge_table, int loops,
                                             int wl_iter, int half_iter, uint64_t num_graphs,
                                             const uint32_t *num_nodes, const uint32_t *edges,
                                             const uint64_t *edge_offsets, const uint32_t *node_labels,
                                             const uint32_t *edge_labels, const uint8_t *in, uint64_t in_len,
                                             const uint64_t *in_offsets, const uint64_t *in_lens, uint32_t *perm,
                                             uint8_t *out, uint64_t out_cap, uint64_t *offsets, uint64_t *lens,
                                             uint64_t *total);
int ans_gpu_ar_polya_wl_labelled_pop_graphs(ans_gpu_tableset *ts, uint32_t node_table, uint32_t edge_table, int loops,
                                            int wl_iter, int half_iter, uint64_t num_graphs, const uint32_t *num_nodes,
                                            const uint64_t *edge_offsets, const uint8_t *in, uint64_t in_len,
                                            const uint64_t *in_offsets, const uint64_t *in_lens, uint32_t *out_edges,
                                            uint32_t *out_num_edges, uint32_t *out_node_labels,
                                            uint32_t *out_edge_labels, uint8_t *out, uint64_t out_cap, uint64_t *offsets,
                                            uint64_t *lens, uint64_t *total);

/* ======================================================================
 * (5h) Joint shuffle coding of graphs in bulk: ans_joint_er_wl_push / _pop and ans_joint_polya_wl_push /
 *      _pop (section 3) of graph g onto / from the message ALREADY in slot g, one lane per graph, under
 *      the resume contract exactly as section 5f has it (slots, d_lens, d_perm, d_num_edges, the
 *      statuses OR-ed into *d_status with d_lens[g] = 0 for the failing graph alone).  The bytes equal
 *      the host codec's.  wl_iter above ANS_WL_MAX_ITER is ANS_E_ARG.  On an Erdős–Rényi pop the
 *      offsets are CAPACITIES and a graph's state holds min(capacity, max_edges) pairs; one more is
 *      ANS_E_LEN for that graph.  On a Pólya urn pop the offsets give each graph's pair count (the
 *      codec's parameter; more than max_edges is ANS_E_ARG for that graph) and d_num_edges[g]
 *      receives it back, 0 for a failing graph.
 *      Slack: a push's orbit pops add nothing and its ordered push what the ordered codec's bound says;
 *      a pop's orbit pushes add at most bitlen(max_nodes) bits each.  ans_gpu_joint_er_slack equals
 *      ans_gpu_ar_er_slack (the same indicators on a push, the same orbit pushes on a pop);
 *      ans_gpu_joint_polya_slack is ans_gpu_polya_slack plus max_nodes * bitlen(max_nodes) / 8 + 1 +
 *      (max_nodes >> 20) bytes.  With slot_cap >= d_lens[g] + that slack
 *      neither call meets ANS_E_LEN for a slot.  The host-buffer calls apply it.
 *      The per-lane state, with K = wl_iter + 1: the orbit stage is 5f's but for its dirty list, which
 *      holds one position at wl_iter = 0 (an update starts from one position): o = (2K + 6) max_nodes
 *      dwords at wl_iter > 0 and 5 max_nodes + 1 at wl_iter = 0 (0 without nodes).  The ordered codec
 *      and the orbit stage never run at the same time, so the urn's arrays (section 5c) lie over the orbit
 *      stage's: u = 2 max_nodes + 6 max_edges + 2 dwords on a push and 2 max_nodes + 5 max_edges + 2 +
 *      min(max_edges, 11) on a pop.  Erdős–Rényi push 3 max_nodes + 2 max_edges + 1 + o, pop
 *      2 max_nodes + 2 max_edges + o; Pólya urn push 3 max_nodes + 2 max_edges + 1 + max(o, u), pop
 *      max(2 max_nodes + 2 max_edges + o, u).  The same 256 MiB rule holds.
 *      Kernel names in ans_gpu_last_launch: k_joint_er_push(wl_iter=1,half_iter=1), k_joint_er_pop(..),
 *      k_joint_pu_push(wl_iter=1,half_iter=1,redraws=0), k_joint_pu_pop(..).
 * ====================================================================== */
int ans_gpu_joint_er_slack(const ans_gpu_table *gt, uint32_t max_nodes, int loops, uint64_t *bytes);
int ans_gpu_joint_polya_slack(uint32_t max_nodes, uint64_t max_edges, uint64_t *bytes);
int ans_dev_joint_er_wl_push(ans_gpu_table *gt, int loops, int wl_iter, int half_iter, uint64_t num_graphs,
                             const uint32_t *d_num_nodes, const uint32_t *d_edges, const uint64_t *d_edge_offsets,
                             uint32_t max_nodes, uint64_t max_edges, uint32_t *d_perm /* NULL or num_graphs * max_nodes */,
                             uint8_t *d_slots, uint64_t slot_cap, uint32_t *d_lens /* in/out */, uint32_t *d_status,
                             void *stream);
int ans_dev_joint_er_wl_pop(ans_gpu_table *gt, int loops, int wl_iter, int half_iter, uint64_t num_graphs,
                            const uint32_t *d_num_nodes, uint32_t *d_edges /* out */,
                            const uint64_t *d_edge_offsets /* capacities */, uint32_t *d_num_edges /* out */,
                            uint32_t max_nodes, uint64_t max_edges, uint8_t *d_slots /* in/out */, uint64_t slot_cap,
                            uint32_t *d_lens /* in/out */, uint32_t *d_status, void *stream);
int ans_dev_joint_polya_wl_push(ans_gpu *g, int loops, int redraws, int wl_iter, int half_iter, uint64_t num_graphs,
                                const uint32_t *d_num_nodes, const uint32_t *d_edges, const uint64_t *d_edge_offsets,
                                uint32_t max_nodes, uint64_t max_edges, uint32_t *d_perm, uint8_t *d_slots,
                                uint64_t slot_cap, uint32_t *d_lens /* in/out */, uint32_t *d_status, void *stream);
int ans_dev_joint_polya_wl_pop(ans_gpu *g, int loops, int redraws, int wl_iter, int half_iter, uint64_t num_graphs,
                               const uint32_t *d_num_nodes, uint32_t *d_edges /* out */,
                               const uint64_t *d_edge_offsets /* the pair counts */, uint32_t *d_num_edges /* out */,
                               uint32_t max_nodes, uint64_t max_edges, uint8_t *d_slots /* in/out */, uint64_t slot_cap,
                               uint32_t *d_lens /* in/out */, uint32_t *d_status, void *stream);
/* ... on host buffers, synchronous, exactly as ans_gpu_ar_er_wl_push_graphs / _pop_graphs. */
int ans_gpu_joint_er_wl_push_graphs(ans_gpu_table *gt, int loops, int wl_iter, int half_iter, uint64_t num_graphs,
                                    const uint32_t *num_nodes, const uint32_t *edges, const uint64_t *edge_offsets,
                                    const uint8_t *in, uint64_t in_len, const uint64_t *in_offsets,
                                    const uint64_t *in_lens, uint32_t *perm, uint8_t *out, uint64_t out_cap,
                                    uint64_t *offsets, uint64_t *lens, uint64_t *total);
int ans_gpu_joint_er_wl_pop_graphs(ans_gpu_table *gt, int loops, int wl_iter, int half_iter, uint64_t num_graphs,
                                   const uint32_t *num_nodes, const uint64_t *edge_offsets, const uint8_t *in,
                                   uint64_t in_len, const uint64_t *in_offsets, const uint64_t *in_lens,
                                   uint32_t *out_edges, uint32_t *out_num_edges, uint8_t *out, uint64_t out_cap,
                                   uint64_t *offsets, uint64_t *lens, uint64_t *total);
int ans_gpu_joint_polya_wl_push_graphs(ans_gpu *g, int loops, int redraws, int wl_iter, int half_iter,
                                       uint64_t num_graphs, const uint32_t *num_nodes, const uint32_t *edges,
                                       const uint64_t *edge_offsets, const uint8_t *in, uint64_t in_len,
                                       const uint64_t *in_offsets, const uint64_t *in_lens, uint32_t *perm,
                                       uint8_t *out, uint64_t out_cap, uint64_t *offsets, uint64_t *lens,
                                       uint64_t *total);
int ans_gpu_joint_polya_wl_pop_graphs(ans_gpu *g, int loops, int redraws, int wl_iter, int half_iter,
                                      uint64_t num_graphs, const uint32_t *num_nodes, const uint64_t *edge_offsets,
                                      const uint8_t *in, uint64_t in_len, const uint64_t *in_offsets,
                                      const uint64_t *in_lens, uint32_t *out_edges, uint32_t *out_num_edges,
                                      uint8_t *out, uint64_t out_cap, uint64_t *offsets, uint64_t *lens,
                                      uint64_t *total);

#ifdef __cplusplus
}
#endif
#endif /* ANS_CAPI_H */
