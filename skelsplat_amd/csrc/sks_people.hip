// sks_people.hip -- several people in front of the sequence pipeline, for MI355X: which detections of a frame's views show the same
// person (sks_associate_people) and which person of a frame is which person of the frame before (sks_track_people).  Both rules,
// with the order of every sum, stand in include/skelsplat_hip.h above the prototypes ("People"); this file follows them op by op in
// float64 and is compiled without FMA contraction like the rest of the library, so a frame's bits are the same wherever it is
// computed.  No global atomics and no floating-point atomics: the only atomics are integer ones on LDS words (an edge's slot in
// the unsorted list, a bit of the veto matrix, two counters), none of which can change a result -- the list is sorted by a total
// order afterwards, an OR and a count do not depend on the order of their operands.
//
// k_associate.  One workgroup of 256 threads per frame; everything but the detections lives in LDS (people_lds):
//   1. the 2x2 minors of every view's projection matrix (18 doubles a view), from which any pair's fundamental matrix is eleven
//      multiplications and five additions an entry -- computed in the frame's own workgroup for a shared rig and for a rig per
//      frame alike, so the bits are the same either way;
//   2. the pair costs, spread over the threads (thread t takes the pairs t, t + 256, ..); an edge goes into the list (cost bits,
//      a * 128 + b), a veto sets two bits of the D x D veto matrix (2 KB at D = 128);
//   3. one bitonic sort of the list in LDS on (cost bits, a, b), padded to the next power of two of the frame's own edge count --
//      one sorter for every length, so there is no regime to switch;
//   4. the merge walk, sequential over the edges, by the first wavefront: lane l owns detections l and l + 64; a cluster is
//      labelled by its lowest member and carries a 128-bit member mask and a 64-bit view mask, so "same cluster" is one compare,
//      "share a view" one AND, and the veto test one AND per member, across the lanes, and a ballot;
//   5. the people: every root ranks itself against the others, the first K are written, and the gathered detections and the
//      clusters' mean edge costs leave from the same launch.
// k_track.  One wavefront (a workgroup of 64 threads) per recording, walking its frames in order; lane = slot * 8 + person.  The
//   slots' last matched poses live in LDS (3 KB), a slot's state (alive, age, id) in the registers of its eight lanes.  The greedy
//   matching takes the smallest live (cost, slot, person) by a butterfly over the cost bits and a ballot, at most eight times.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/skelsplat_hip.h"
#include "sks_err.h"

namespace {

typedef unsigned long long u64;

constexpr int THREADS = 256;
constexpr int TRACK_THREADS = 64;
constexpr int MAXD = SKS_PEOPLE_MAX_DETS;
constexpr int MAXK = SKS_PEOPLE_MAX;
constexpr int MAXM = SKS_PEOPLE_MAX_SLOTS;
static_assert(MAXD == 128 && MAXK == 8, "lane l owns detections l and l + 64; eight slots x eight people are the 64 lanes");

// The LDS of k_associate for V views of M slots, in this order: u64 / double words, then ints, then the edges' (a, b) shorts.
struct PeopleLds {
    int cap;            // entries of the edge list: the next power of two of M^2 V (V - 1) / 2, at least 2
    size_t minors;      // [V][3][6] doubles
    size_t veto;        // [D][2] u64: bit b of row a = the pair (a, b) is a veto
    size_t members;     // [D][2] u64: the members of the cluster labelled i
    size_t views;       // [D] u64: its views
    size_t keys;        // [cap] u64: the edges' cost bits; afterwards the pair costs of one person, [V (V - 1) / 2] doubles
    size_t label;       // [D] ints: the cluster of detection i (its lowest member)
    size_t live;        // [D] ints: detection i has a usable joint
    size_t slot_of;     // [D] ints: the person slot of the cluster labelled i, or -1
    size_t assign;      // [MAXK][V] ints
    size_t person;      // [MAXK] ints: the label of person k, or -1
    size_t misc;        // [4] ints: edges, people, unassigned, padded length
    size_t ab;          // [cap] shorts
    size_t bytes;
};

__host__ __device__ inline PeopleLds people_lds(int V, int M)
{
    PeopleLds l;
    const int D = V * M;
    const int emax = M * M * (V * (V - 1) / 2);
    int cap = 2;
    while (cap < emax) cap <<= 1;
    l.cap = cap;
    size_t at = 0;
    l.minors = at;  at += (size_t)V * 18 * 8;
    l.veto = at;    at += (size_t)D * 2 * 8;
    l.members = at; at += (size_t)D * 2 * 8;
    l.views = at;   at += (size_t)D * 8;
    l.keys = at;    at += (size_t)cap * 8;
    l.label = at;   at += (size_t)D * 4;
    l.live = at;    at += (size_t)D * 4;
    l.slot_of = at; at += (size_t)D * 4;
    l.assign = at;  at += (size_t)MAXK * V * 4;
    l.person = at;  at += (size_t)MAXK * 4;
    l.misc = at;    at += 4 * 4;
    l.ab = at;      at += (size_t)cap * 2;
    l.bytes = (at + 15) & ~(size_t)15;
    return l;
}

// The six 2x2 minors of rows r0 < r1 of a 3x4 matrix, columns (0,1) (0,2) (0,3) (1,2) (1,3) (2,3)
__device__ __forceinline__ void minors6(const double* r0, const double* r1, double* m)
{
    m[0] = r0[0] * r1[1] - r0[1] * r1[0];
    m[1] = r0[0] * r1[2] - r0[2] * r1[0];
    m[2] = r0[0] * r1[3] - r0[3] * r1[0];
    m[3] = r0[1] * r1[2] - r0[2] * r1[1];
    m[4] = r0[1] * r1[3] - r0[3] * r1[1];
    m[5] = r0[2] * r1[3] - r0[3] * r1[2];
}

// F of views va < vb from their minors, row-major F[3 j + i]: the header's Laplace expansion along the first two rows
__device__ __forceinline__ void fundamental(const double* minors, int va, int vb, double* F)
{
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const double* B = minors + (vb * 3 + j) * 6;
#pragma unroll
        for (int i = 0; i < 3; i++) {
            const double* A = minors + (va * 3 + i) * 6;
            const double det = ((((A[0] * B[5] - A[1] * B[4]) + A[2] * B[3]) + A[3] * B[2]) - A[4] * B[1]) + A[5] * B[0];
            F[3 * j + i] = ((i + j) & 1) ? -det : det;
        }
    }
}

// The header's pair cost of detections a (xa, kept by ka) and b: true when the pair is measured, c = its cost
template <typename T>
__device__ __forceinline__ bool pair_cost(const double* F, const T* xa, const T* xb, const unsigned char* ka, const unsigned char* kb,
                                          int J, int min_joints, double& c)
{
    double sum = 0.0;
    int n = 0;
    for (int j = 0; j < J; j++) {
        if (ka && (ka[j] == 0 || kb[j] == 0)) continue;
        const double ax = (double)xa[2 * j], ay = (double)xa[2 * j + 1], bx = (double)xb[2 * j], by = (double)xb[2 * j + 1];
        if (!(isfinite(ax) && isfinite(ay) && isfinite(bx) && isfinite(by))) continue;
        const double l0 = (F[0] * ax + F[1] * ay) + F[2];
        const double l1 = (F[3] * ax + F[4] * ay) + F[5];
        const double l2 = (F[6] * ax + F[7] * ay) + F[8];
        const double db = fabs((l0 * bx + l1 * by) + l2) / sqrt(l0 * l0 + l1 * l1);
        const double t0 = (F[0] * bx + F[3] * by) + F[6];
        const double t1 = (F[1] * bx + F[4] * by) + F[7];
        const double t2 = (F[2] * bx + F[5] * by) + F[8];
        const double da = fabs((t0 * ax + t1 * ay) + t2) / sqrt(t0 * t0 + t1 * t1);
        const double d = 0.5 * (db + da);
        if (!isfinite(d)) continue;
        sum = sum + d;
        n++;
    }
    c = sum / (double)n;
    return n >= min_joints;
}

template <typename T>
struct PeopleArgs {
    int N, V, M, J, K;
    const double* proj;
    size_t rig_stride;
    const T* det;
    const unsigned char* valid;
    double max_px;
    int min_joints, min_views;
    int* assign;
    int* n_people;
    int* n_overflow;
    int* n_unassigned;
    double* cost;
    T* gathered;
};

template <typename T>
__global__ void __launch_bounds__(THREADS) k_associate(PeopleArgs<T> p)
{
    extern __shared__ u64 s_mem[];
    const int V = p.V, M = p.M, J = p.J, K = p.K, D = V * M;
    const PeopleLds L = people_lds(V, M);
    char* base = reinterpret_cast<char*>(s_mem);
    double* s_minors = reinterpret_cast<double*>(base + L.minors);
    u64* s_veto = reinterpret_cast<u64*>(base + L.veto);
    u64* s_members = reinterpret_cast<u64*>(base + L.members);
    u64* s_views = reinterpret_cast<u64*>(base + L.views);
    u64* s_keys = reinterpret_cast<u64*>(base + L.keys);
    int* s_label = reinterpret_cast<int*>(base + L.label);
    int* s_live = reinterpret_cast<int*>(base + L.live);
    int* s_slot_of = reinterpret_cast<int*>(base + L.slot_of);
    int* s_assign = reinterpret_cast<int*>(base + L.assign);
    int* s_person = reinterpret_cast<int*>(base + L.person);
    int* s_misc = reinterpret_cast<int*>(base + L.misc);
    unsigned short* s_ab = reinterpret_cast<unsigned short*>(base + L.ab);
    const int tid = threadIdx.x;
    const size_t f = blockIdx.x;
    const double* P = p.proj + f * p.rig_stride;
    const T* det = p.det + f * (size_t)D * J * 2;
    const unsigned char* valid = p.valid ? p.valid + f * (size_t)D * J : nullptr;

    // 1. the views' minors; the singletons
    for (int t = tid; t < 3 * V; t += THREADS) {
        const int v = t / 3, i = t - 3 * v;
        const double* Pv = P + (size_t)v * 12;
        minors6(Pv + 4 * (i == 0 ? 1 : 0), Pv + 4 * (i == 2 ? 1 : 2), s_minors + (size_t)t * 6);
    }
    for (int i = tid; i < D; i += THREADS) {
        s_veto[2 * i] = 0; s_veto[2 * i + 1] = 0;
        s_members[2 * i] = i < 64 ? 1ull << i : 0ull;
        s_members[2 * i + 1] = i < 64 ? 0ull : 1ull << (i - 64);
        s_views[i] = 1ull << (i / M);
        s_label[i] = i;
        s_slot_of[i] = -1;
        int live = 0;
        for (int j = 0; j < J; j++) {
            const double x = (double)det[((size_t)i * J + j) * 2], y = (double)det[((size_t)i * J + j) * 2 + 1];
            if ((!valid || valid[(size_t)i * J + j] != 0) && isfinite(x) && isfinite(y)) { live = 1; break; }
        }
        s_live[i] = live;
    }
    if (tid < MAXK) s_person[tid] = -1;
    if (tid < 4) s_misc[tid] = 0;
    __syncthreads();

    // 2. the pair costs: edges into the list, vetoes into the matrix
    for (int q = tid; q < D * D; q += THREADS) {
        const int a = q / D, b = q - a * D;
        const int va = a / M, vb = b / M;
        if (va >= vb) continue;
        double F[9], c;
        fundamental(s_minors, va, vb, F);
        const bool measured = pair_cost<T>(F, det + (size_t)a * J * 2, det + (size_t)b * J * 2, valid ? valid + (size_t)a * J : nullptr,
                                           valid ? valid + (size_t)b * J : nullptr, J, p.min_joints, c);
        if (!measured) continue;
        if (c <= p.max_px) {
            const int at = atomicAdd(&s_misc[0], 1);            // (at most one entry a pair: at < M^2 V (V - 1) / 2 <= cap)
            s_keys[at] = (u64)__double_as_longlong(c);          // (c >= +0 and finite: its bit pattern orders like its value)
            s_ab[at] = (unsigned short)(a * MAXD + b);
        } else {
            atomicOr(&s_veto[2 * a + (b >> 6)], 1ull << (b & 63));
            atomicOr(&s_veto[2 * b + (a >> 6)], 1ull << (a & 63));
        }
    }
    __syncthreads();

    // 3. the list in ascending (cost, a, b): bitonic, padded with keys no edge has
    const int n_e = s_misc[0];
    int n2 = 1;
    while (n2 < n_e) n2 <<= 1;
    for (int i = n_e + tid; i < n2; i += THREADS) { s_keys[i] = ~0ull; s_ab[i] = 0xffff; }
    __syncthreads();
    for (int k = 2; k <= n2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < n2; i += THREADS) {
                const int x = i ^ j;
                if (x <= i) continue;
                const u64 ki = s_keys[i], kx = s_keys[x];
                const unsigned short pi = s_ab[i], px = s_ab[x];
                const bool after = ki > kx || (ki == kx && pi > px);
                if (after == ((i & k) == 0)) { s_keys[i] = kx; s_keys[x] = ki; s_ab[i] = px; s_ab[x] = pi; }
            }
            __syncthreads();
        }
    }

    // 4. the merge walk, by the first wavefront: every lane reads the same edge and the same two clusters
    if (tid < 64) {
        const int lane = tid;
        volatile int* label = s_label;
        volatile u64* members = s_members;
        volatile u64* views = s_views;
        for (int e = 0; e < n_e; e++) {
            const int ab = __builtin_amdgcn_readfirstlane((int)s_ab[e]);
            const int a = ab / MAXD, b = ab % MAXD;
            const int la = __builtin_amdgcn_readfirstlane(label[a]), lb = __builtin_amdgcn_readfirstlane(label[b]);
            if (la == lb) continue;
            const u64 wa = views[la], wb = views[lb];
            if (wa & wb) continue;
            const u64 a0 = members[2 * la], a1 = members[2 * la + 1], b0 = members[2 * lb], b1 = members[2 * lb + 1];
            bool hit = false;
            if ((a0 >> lane) & 1ull) hit = ((s_veto[2 * lane] & b0) | (s_veto[2 * lane + 1] & b1)) != 0ull;
            if ((a1 >> lane) & 1ull) hit = hit || ((s_veto[2 * (lane + 64)] & b0) | (s_veto[2 * (lane + 64) + 1] & b1)) != 0ull;
            if (__ballot(hit ? 1 : 0) != 0ull) continue;
            const int keep = la < lb ? la : lb;
            const u64 d0 = la < lb ? b0 : a0, d1 = la < lb ? b1 : a1;       // the members that change their label
            if ((d0 >> lane) & 1ull) label[lane] = keep;
            if ((d1 >> lane) & 1ull) label[lane + 64] = keep;
            if (lane == 0) {
                members[2 * keep] = a0 | b0;
                members[2 * keep + 1] = a1 | b1;
                views[keep] = wa | wb;
            }
            __builtin_amdgcn_wave_barrier();
        }
    }
    __syncthreads();

    // 5. the people: clusters of min_views members, by member count descending, then by label
    for (int i = tid; i < D; i += THREADS) {
        if (s_label[i] != i) continue;
        const int ci = __popcll(s_members[2 * i]) + __popcll(s_members[2 * i + 1]);
        if (ci < p.min_views) continue;
        int rank = 0;
        for (int o = 0; o < D; o++) {
            if (o == i || s_label[o] != o) continue;
            const int co = __popcll(s_members[2 * o]) + __popcll(s_members[2 * o + 1]);
            if (co >= p.min_views && (co > ci || (co == ci && o < i))) rank++;
        }
        atomicAdd(&s_misc[1], 1);
        if (rank < K) { s_person[rank] = i; s_slot_of[i] = rank; }
    }
    __syncthreads();
    for (int t = tid; t < K * V; t += THREADS) {
        const int k = t / V, v = t - k * V;
        const int root = s_person[k];
        int slot = -1;
        if (root >= 0) {
            for (int m = 0; m < M; m++) {
                const int i = v * M + m;
                if ((s_members[2 * root + (i >> 6)] >> (i & 63)) & 1ull) slot = m;      // (one member a view at most)
            }
        }
        s_assign[t] = slot;
        p.assign[(f * K + k) * V + v] = slot;
    }
    for (int i = tid; i < D; i += THREADS)
        if (s_live[i] && s_slot_of[s_label[i]] < 0) atomicAdd(&s_misc[2], 1);
    __syncthreads();
    if (tid == 0) {
        const int people = s_misc[1];
        p.n_people[f] = people < K ? people : K;
        p.n_overflow[f] = people < K ? 0 : people - K;
        p.n_unassigned[f] = s_misc[2];
    }

    // the gathered detections: the input's own bits where the person has a detection and the joint is kept, NaN elsewhere
    T* out = p.gathered + f * (size_t)K * V * J * 2;
    for (int t = tid; t < K * V * J; t += THREADS) {
        const int kv = t / J, j = t - kv * J;
        const int v = kv % V;
        const int slot = s_assign[kv];
        T x = (T)NAN, y = (T)NAN;
        if (slot >= 0) {
            const size_t at = (size_t)(v * M + slot) * J + j;
            if (!valid || valid[at] != 0) { x = det[2 * at]; y = det[2 * at + 1]; }
        }
        out[2 * (size_t)t] = x;
        out[2 * (size_t)t + 1] = y;
    }

    // the clusters' mean edge costs: the pair costs of one person side by side (over the list, which is spent), then one
    // thread adds them in ascending (a, b) = ascending (va, vb)
    double* s_pair = reinterpret_cast<double*>(s_keys);
    const int n_pairs = V * (V - 1) / 2;
    for (int k = 0; k < K; k++) {
        __syncthreads();
        if (s_person[k] < 0) {
            if (tid == 0) p.cost[f * K + k] = (double)NAN;
            continue;                                               // (read from LDS: the whole workgroup skips together)
        }
        for (int q = tid; q < V * V; q += THREADS) {
            const int va = q / V, vb = q - va * V;
            if (va >= vb) continue;
            const int ma = s_assign[k * V + va], mb = s_assign[k * V + vb];
            double c = -1.0;
            if (ma >= 0 && mb >= 0) {
                const int a = va * M + ma, b = vb * M + mb;
                double F[9], cc;
                fundamental(s_minors, va, vb, F);
                if (pair_cost<T>(F, det + (size_t)a * J * 2, det + (size_t)b * J * 2, valid ? valid + (size_t)a * J : nullptr,
                                 valid ? valid + (size_t)b * J : nullptr, J, p.min_joints, cc) && cc <= p.max_px)
                    c = cc;
            }
            s_pair[va * V - va * (va + 1) / 2 + (vb - va - 1)] = c;
        }
        __syncthreads();
        if (tid == 0) {
            double sum = 0.0;
            int n = 0;
            for (int q = 0; q < n_pairs; q++) {
                const double c = s_pair[q];
                if (c >= 0.0) { sum = sum + c; n++; }
            }
            p.cost[f * K + k] = n > 0 ? sum / (double)n : (double)NAN;
        }
    }
}

__device__ __forceinline__ bool finite3(const float* x) { return isfinite(x[0]) && isfinite(x[1]) && isfinite(x[2]); }

__global__ void __launch_bounds__(TRACK_THREADS)
k_track(int N, int K, int J, const float* __restrict__ joints, const int* __restrict__ groups, double max_mm, int max_gap,
        int min_joints, int* __restrict__ track_id, int* __restrict__ n_tracks, int* __restrict__ n_dropped)
{
    __shared__ float s_pose[MAXK][SKS_MAX_CHANNELS * 3];
    const int lane = threadIdx.x, s = lane >> 3, k = lane & 7;
    const int g = blockIdx.x;
    int alive = 0, age = 0, id = -1;                // of slot s, the same in its eight lanes
    int next_id = 0, dropped = 0;
    for (int f = 0; f < N; f++) {
        if ((groups ? groups[f] : 0) != g) continue;
        const float* pf = joints + (size_t)f * K * J * 3;
        // person k: present with min_joints finite joints
        int n_fin = 0;
        if (k < K)
            for (int j = 0; j < J; j++) n_fin += finite3(pf + ((size_t)k * J + j) * 3) ? 1 : 0;
        const bool present = k < K && n_fin >= min_joints;
        // the cost of (slot s, person k)
        bool ok = false;
        double c = 0.0;
        if (alive && present) {
            double sum = 0.0;
            int n = 0;
            for (int j = 0; j < J; j++) {
                const float* a = pf + ((size_t)k * J + j) * 3;
                const float* b = s_pose[s] + 3 * j;
                if (!finite3(a) || !finite3(b)) continue;
                const double dx = (double)a[0] - (double)b[0], dy = (double)a[1] - (double)b[1], dz = (double)a[2] - (double)b[2];
                sum = sum + sqrt((dx * dx + dy * dy) + dz * dz);
                n++;
            }
            if (n >= min_joints) {
                c = sum / (double)n;
                ok = c <= max_mm;
            }
        }
        // greedy, one to one, in ascending (cost, s, k): the smallest live key, its first lane
        unsigned taken_s = 0, taken_k = 0;
        int person_of_slot = -1, slot_of_person = -1;
        for (int round = 0; round < MAXK; round++) {
            const bool live = ok && !((taken_s >> s) & 1u) && !((taken_k >> k) & 1u);
            if (__ballot(live ? 1 : 0) == 0ull) break;
            const u64 key = live ? (u64)__double_as_longlong(c) : ~0ull;     // (c >= +0 and finite: the bits order like the value)
            u64 best = key;
            for (int m = 1; m < 64; m <<= 1) {
                const u64 o = (u64)__shfl_xor((long long)best, m, 64);
                best = o < best ? o : best;
            }
            const int who = __ffsll((long long)__ballot(live && key == best ? 1 : 0)) - 1;
            const int ws = who >> 3, wk = who & 7;
            taken_s |= 1u << ws;
            taken_k |= 1u << wk;
            if (ws == s) person_of_slot = wk;
            if (wk == k) slot_of_person = ws;
        }
        // matched people take their slot's id; unmatched slots age and are freed before any track opens
        const int id_of_match = __shfl(id, (slot_of_person < 0 ? 0 : slot_of_person) * 8, 64);
        int my_id = slot_of_person >= 0 ? id_of_match : -1;
        int src = person_of_slot;                   // the person whose pose slot s takes in this frame, or -1
        if (alive) {
            if (person_of_slot >= 0) age = 0;
            else if (++age > max_gap) alive = 0;
        }
        const u64 free_lanes = __ballot(k == 0 && !alive ? 1 : 0);                          // bit 8 s: slot s is free
        const unsigned open = (unsigned)__ballot(s == 0 && present && slot_of_person < 0 ? 1 : 0) & 0xffu;      // bit k: person k opens
        const int n_free = __popcll(free_lanes), n_open = __popc(open);
        for (int kk = 0; kk < K; kk++) {
            if (!((open >> kk) & 1u)) continue;
            const int r = __popc(open & ((1u << kk) - 1u));
            if (r >= n_free) continue;
            u64 rest = free_lanes;
            for (int i = 0; i < r; i++) rest &= rest - 1ull;
            const int slot = (__ffsll((long long)rest) - 1) >> 3;
            if (slot == s) { alive = 1; age = 0; id = next_id + r; src = kk; }
            if (kk == k) my_id = next_id + r;
        }
        next_id += n_open < n_free ? n_open : n_free;
        dropped += n_open > n_free ? n_open - n_free : 0;
        if (s == 0 && k < K) track_id[(size_t)f * K + k] = my_id;
        __syncthreads();                            // every cost of this frame is read
        if (src >= 0)
            for (int e = k; e < J * 3; e += 8) s_pose[s][e] = pf[(size_t)src * J * 3 + e];
        __syncthreads();
    }
    if (lane == 0) { n_tracks[g] = next_id; n_dropped[g] = dropped; }
}

int check_people(const char* who, int N, int V, int M, int J, int K)
{
    if (N < 1 || N > (1 << 26)) return fail2(-1, "%s: N = %d frames, 1 .. 2^26", who, N);
    if (V < 1 || V > SKS_MAX_VIEWS) return fail2(-1, "%s: V = %d views, 1 .. %d (SKS_MAX_VIEWS)", who, V, SKS_MAX_VIEWS);
    if (M < 1 || M > MAXM) return fail2(-1, "%s: M = %d candidates a view, 1 .. %d (SKS_PEOPLE_MAX_SLOTS)", who, M, MAXM);
    if (V * M > MAXD) return fail2(-1, "%s: V * M = %d detections a frame, at most %d (SKS_PEOPLE_MAX_DETS)", who, V * M, MAXD);
    if (J < 1 || J > SKS_MAX_CHANNELS) return fail2(-1, "%s: J = %d joints, 1 .. %d (SKS_MAX_CHANNELS)", who, J, SKS_MAX_CHANNELS);
    if (K < 1 || K > MAXK) return fail2(-1, "%s: K = %d people, 1 .. %d (SKS_PEOPLE_MAX)", who, K, MAXK);
    return 0;
}

template <typename T>
int launch_associate(const PeopleArgs<T>& a, void* stream)
{
    const size_t lds = people_lds(a.V, a.M).bytes;
    if (lds > 48 * 1024)        // gfx950 has 160 KB of LDS per CU; raise the per-kernel dynamic limit for the long lists
        HIP_TRY2(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_associate<T>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k_associate<T>, dim3(a.N), dim3(THREADS), lds, (hipStream_t)stream, a);
    HIP_TRY2(hipGetLastError());
    return 0;
}

}  // namespace

extern "C" int sks_people_launch(int V, int M, int* out)
{
    if (int rc = check_people("people_launch", 1, V, M, 1, 1)) return rc;
    if (!out) return fail2(-2, "people_launch: missing out (SKS_PEOPLE_LAUNCH_INTS ints)");
    const PeopleLds l = people_lds(V, M);
    out[SKS_PEOPLE_ASSOC_THREADS] = THREADS;
    out[SKS_PEOPLE_ASSOC_LDS_BYTES] = (int)l.bytes;
    out[SKS_PEOPLE_ASSOC_LIST_ENTRIES] = l.cap;
    out[SKS_PEOPLE_TRACK_THREADS] = TRACK_THREADS;
    return 0;
}

extern "C" int sks_associate_people(int N, int V, int M, int J, int K, const double* proj, size_t rig_stride, const float* detections,
                                    const double* detections_f64, const unsigned char* valid, double max_px, int min_joints,
                                    int min_views, int* assign, int* n_people, int* n_overflow, int* n_unassigned, double* cost,
                                    float* gathered, double* gathered_f64, void* stream)
{
    if (int rc = check_people("associate_people", N, V, M, J, K)) return rc;
    if (!proj) return fail2(-2, "associate_people: missing proj ((V,3,4) or (N,V,3,4) doubles)");
    if (rig_stride != 0 && rig_stride != (size_t)V * 12) return fail2(-1, "associate_people: rig_stride must be 0 or V * 12 = %d", V * 12);
    if ((detections != nullptr) == (detections_f64 != nullptr))
        return fail2(-2, "associate_people: exactly one of detections (float) and detections_f64 (double)");
    if ((detections != nullptr) != (gathered != nullptr) || (detections_f64 != nullptr) != (gathered_f64 != nullptr))
        return fail2(-2, "associate_people: the gathered detections leave in the input's type (gathered with detections, gathered_f64 with detections_f64)");
    if (!(max_px >= 0.0) || !isfinite(max_px)) return fail2(-1, "associate_people: max_px must be finite and >= 0 pixels, got %g", max_px);
    if (min_joints < 1 || min_joints > J) return fail2(-1, "associate_people: min_joints = %d, 1 .. J = %d", min_joints, J);
    if (min_views < 2 || min_views > SKS_MAX_VIEWS) return fail2(-1, "associate_people: min_views = %d, 2 .. %d (SKS_MAX_VIEWS)", min_views, SKS_MAX_VIEWS);
    if (!assign || !n_people || !n_overflow || !n_unassigned || !cost)
        return fail2(-2, "associate_people: missing assign (N,K,V) / n_people / n_overflow / n_unassigned (N) ints or cost (N,K) doubles");
    if (people_lds(V, M).bytes > 160 * 1024) return fail2(-1, "associate_people: V = %d, M = %d needs more than 160 KiB of LDS", V, M);
    if (detections) {
        const PeopleArgs<float> a = {N, V, M, J, K, proj, rig_stride, detections, valid, max_px, min_joints, min_views,
                                     assign, n_people, n_overflow, n_unassigned, cost, gathered};
        return launch_associate<float>(a, stream);
    }
    const PeopleArgs<double> a = {N, V, M, J, K, proj, rig_stride, detections_f64, valid, max_px, min_joints, min_views,
                                  assign, n_people, n_overflow, n_unassigned, cost, gathered_f64};
    return launch_associate<double>(a, stream);
}

extern "C" int sks_track_people(int N, int K, int J, const float* joints, const int* groups, int n_groups, double max_mm, int max_gap,
                                int min_joints, int* track_id, int* n_tracks, int* n_dropped, void* stream)
{
    if (N < 1 || N > (1 << 26)) return fail2(-1, "track_people: N = %d frames, 1 .. 2^26", N);
    if (K < 1 || K > MAXK) return fail2(-1, "track_people: K = %d people, 1 .. %d (SKS_PEOPLE_MAX)", K, MAXK);
    if (J < 1 || J > SKS_MAX_CHANNELS) return fail2(-1, "track_people: J = %d joints, 1 .. %d (SKS_MAX_CHANNELS)", J, SKS_MAX_CHANNELS);
    if (n_groups < 1 || n_groups > SKS_PEOPLE_MAX_GROUPS) return fail2(-1, "track_people: n_groups = %d, 1 .. %d (SKS_PEOPLE_MAX_GROUPS)", n_groups, SKS_PEOPLE_MAX_GROUPS);
    if (!groups && n_groups != 1) return fail2(-2, "track_people: n_groups = %d without groups (NULL groups: one recording)", n_groups);
    if (!(max_mm >= 0.0) || !isfinite(max_mm)) return fail2(-1, "track_people: max_mm must be finite and >= 0, got %g", max_mm);
    if (max_gap < 0 || max_gap > (1 << 26)) return fail2(-1, "track_people: max_gap = %d frames, 0 .. 2^26", max_gap);
    if (min_joints < 1 || min_joints > J) return fail2(-1, "track_people: min_joints = %d, 1 .. J = %d", min_joints, J);
    if (!joints) return fail2(-2, "track_people: missing joints (N,K,J,3) floats");
    if (!track_id || !n_tracks || !n_dropped) return fail2(-2, "track_people: missing track_id (N,K) or n_tracks / n_dropped (n_groups) ints");
    // -1 everywhere first: a frame whose id names no recording is walked by nobody
    HIP_TRY2(hipMemsetAsync(track_id, 0xff, (size_t)N * K * sizeof(int), (hipStream_t)stream));
    hipLaunchKernelGGL(k_track, dim3(n_groups), dim3(TRACK_THREADS), 0, (hipStream_t)stream, N, K, J, joints, groups, max_mm, max_gap,
                       min_joints, track_id, n_tracks, n_dropped);
    HIP_TRY2(hipGetLastError());
    return 0;
}
