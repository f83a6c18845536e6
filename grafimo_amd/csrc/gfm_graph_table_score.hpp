// gfm_graph_table_score.hpp -- what the kernels of the scoring tables share: the packed two-strand window score, what a
// window adds to an affinity sum, the sequence tables' edit key, and what is read off a replayed walk (device code only;
// included at the end of graph_extract.hip ahead of the table headers: it uses GraphDev, DelEmit, base_code).
namespace {

// A window over the motif's packed table (global or LDS; word [j * 8 + code]: the '+' score of column j in the low half,
// the '-' score in the high half; a code of 4 .. 7 is no base): the packed sum and how many columns hold no base.
struct WindowSum { unsigned sum, bad; };

// code_at(j) -> the base_code of the window's column j: 0 .. 7, which is what bounds the table index (base_code() masks to
// three bits, and the LDS slices of the sequence kernels hold only its results or 4).  It is called exactly once per j, in
// ascending order: graph_variant_kernel's callable completes its k-mer arrays on the way.
template <class F>
__device__ __forceinline__ WindowSum window_sum(const unsigned *ftab, int W, F code_at)
{
    WindowSum w{0u, 0u};
    for (int j = 0; j < W; ++j) {
        const unsigned c = code_at(j);
        w.sum += ftab[j * 8 + c];
        w.bad += c >> 2;
    }
    return w;
}

// THE RULE for a base that is not A, C, G, T: the k-mer that holds one scores min_val on both strands (one strand at a time
// for a caller that may not need the other)
__device__ __forceinline__ int plus_score(WindowSum w, int min_val) { return w.bad ? min_val : (int)(w.sum & 0xffffu); }
__device__ __forceinline__ int minus_score(WindowSum w, int min_val) { return w.bad ? min_val : (int)(w.sum >> 16); }
struct StrandScores { int plus, minus; };
__device__ __forceinline__ StrandScores strand_scores(WindowSum w, int min_val)
{
    return {plus_score(w, min_val), minus_score(w, min_val)};
}

// what a window adds to a sum: the weights of its two strands' scores.  Scores lie in [0, L): the motif's matrix entries
// are within [0, 1000] (checked when the handle is made) and L = 1000 W + 1.
__device__ __forceinline__ unsigned long long walk_value(const unsigned long long *__restrict__ wtab, WindowSum w, int min_val,
                                                         int forward_only)
{
    const StrandScores s = strand_scores(w, min_val);
    const unsigned long long vp = wtab[s.plus];
    return forward_only ? vp : vp + wtab[s.minus];
}

// The key of a window of the sequence tables (gfm_edit_record_t, the mutation scan's keys; include/grafimo_hip.h):
// bits 8 ..: score + 1 (0: the side has no window); bits 1 .. 7: 64 - rel, rel = the window's start minus the edit's offset
// in -63 .. 63, so that an earlier start gives the larger key; bit 0: the '+' strand.
__device__ __forceinline__ unsigned edit_key(int score, int rel, bool plus)
{
    return (((unsigned)score + 1u) << 8) | ((unsigned)(64 - rel) << 1) | (plus ? 1u : 0u);
}

// a constraint as job_constraint() packs it
__device__ __forceinline__ void unpack_constraint(int v, int &site, int &al)
{
    site = v >> 4;
    al = v & 3;
}

// What a replayed walk (replay_walk) left in its DelEmit and the arrays under it.  The arrays -- km, kr, src, more -- stay
// plain locals of each kernel: gathered in one object with the DelEmit they took all of it to scratch memory, the DelEmit's
// register fields too (144 bytes a lane more in every replaying kernel), as DelEmit's own comments tell of its `more`.
// constraint k as carrier_word() and present_by_bitsets() ask for it
struct ConstraintAt {
    const DelEmit &em;
    __device__ __forceinline__ void operator()(int k, int &site, int &al) const { unpack_constraint(em.get(k), site, al); }
};
// the walk is the reference's: every constraint asks for allele 0
__device__ __forceinline__ bool walk_is_reference(const DelEmit &em)
{
    bool ref = true;
    for (int c = 0; c < em.n_cons; ++c)
        if (em.get(c) & 3) ref = false;
    return ref;
}
// the base code of the walk's column j: a reference base is fetched now, any other was written during the replay
__device__ __forceinline__ unsigned walk_code(const GraphDev &g, const int *src, const uint8_t *km, int j)
{
    return base_code(src[j] >= 0 ? g.ref[src[j]] : km[j]);
}

// (Not here, on measurements -- profiles/table_entries_refactor_ab.txt: the two run kernels' plain-window test, which as a
// function changed the control flow the compiler made of both kernels, 18 and 35 instructions more, and cost
// graph_hapaffinity_kernel 1.2 %; and graph_hapscore_kernel altogether, which keeps its own window loops and min_val selects.)

}  // namespace
