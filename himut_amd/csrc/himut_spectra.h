// k_id83, k_dbs78: the indel and doublet spectra (include/himut_hip.h, himut_id83_classify / himut_dbs78_counts; DESIGN.md
// section 8 row 17).  No counterpart in the reference.  The classes are COSMIC's ID83 and DBS78 in SigProfiler's order; the
// rules that put an allele into a class are this package's own definition and are written out in the header.
//
// Both kernels take k_sbs's shape: one thread per allele, grid-strided, a workgroup-private histogram in LDS, one 64-bit
// atomic per non-zero bin at the end.
//
// k_id83.  An allele is (anchor a, type, length L, inserted bases).  A deletion removes seq[a+1 .. a+L]; an insertion puts
// its bases between seq[a] and seq[a+1].  Letters compare without case; a byte outside ACGTacgt matches nothing, itself
// included.  Nothing is read in front of seq[0] or behind seq[len-1] (no wrap-around, unlike k_sbs).  The allele's
// periodic extent m = l + r is scanned on both sides of the allele as the VCF places it:
//   deletion   r: seq[a+1+L+j] == seq[a+1+j] for j < r        l: seq[a-j] == seq[a+L-j] for j < l
//   insertion  r: seq[a+1+j] == I[j mod L] for j < r          l: seq[a-j] == I[(L-1-j) mod L] for j < l
// which is what shifting the allele left as far as it goes (rotating an insertion's bases) and scanning right finds, so
// the class does not depend on where inside its repeat the allele was placed.  The scan ends at m >= 5L: no class looks
// further, and a thread makes at most 5L <= 320 comparisons.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace himut {

constexpr int ID83_CLASSES = 83, ID83_BINS = 88;       // 83 classes, num_nbase, num_range, three reserved words
constexpr int ID83_NBASE = 83, ID83_RANGE = 84;
constexpr int ID83_MAX_LEN = 64;
constexpr int DBS78_CLASSES = 78, DBS78_BINS = 80;     // 78 classes, a letter outside ACGT, a pair with an unchanged base
constexpr int DBS78_NLETTER = 78, DBS78_UNCHANGED = 79;
constexpr int SPECTRA_NO_CLASS = 255;

// The 78 doublet classes in bin order, reference pair then alternative pair, four letters a class (himut_amd/spectra.py
// holds the labels; tests/test_spectra_cpu.py compares the two).
__device__ const char DBS78_TABLE[DBS78_CLASSES * 4 + 1] =
    "ACCAACCGACCTACGAACGGACGTACTAACTGACTT"
    "ATCAATCCATCGATGAATGCATTA"
    "CCAACCAGCCATCCGACCGGCCGTCCTACCTGCCTT"
    "CGATCGGCCGGTCGTACGTCCGTT"
    "CTAACTACCTAGCTGACTGCCTGGCTTACTTCCTTG"
    "GCAAGCAGGCATGCCAGCCGGCTA"
    "TAATTACGTACTTAGCTAGGTAGT"
    "TCAATCAGTCATTCCATCCGTCCTTCGATCGGTCGT"
    "TGAATGACTGATTGCATGCCTGCTTGGATGGCTGGT"
    "TTAATTACTTAGTTCATTCCTTCGTTGATTGCTTGG";

// byte -> A0 C1 G2 T3 in either case, 4 for anything else
__device__ __forceinline__ int acgt_code(int c) {
    const int u = c & ~0x20;
    return u == 'A' ? 0 : u == 'C' ? 1 : u == 'G' ? 2 : u == 'T' ? 3 : 4;
}

// base i of an indel record's inserted bases (2 bits a base, codes "ATGC") as A0 C1 G2 T3
__device__ __forceinline__ int ins_code(const uint32_t w[4], int i) {
    const int k = (int)(w[i >> 4] >> (2 * (i & 15))) & 3;       // A0 T1 G2 C3
    return k == 1 ? 3 : k == 3 ? 1 : k;
}

// the class of an allele from its type, length, first letter (L = 1) and periodic extent m (capped or not)
__device__ __forceinline__ int id83_class(int type, int L, int letter, int m) {
    if (L == 1) {
        const int t = letter == 0 || letter == 3 ? 6 : 0;      // A and T report as T, C and G as C
        return type * 12 + t + min(m, 5);
    }
    const int size = min(L, 5);
    if (type == 0 && m > 0 && m < L) return (size == 2 ? 72 : size == 3 ? 73 : size == 4 ? 75 : 78) + min(m, 5) - 1;
    return (type == 0 ? 24 : 48) + (size - 2) * 6 + min(m / L, 5);
}

__global__ void __launch_bounds__(256) k_id83(const uint8_t* __restrict__ seq, int64_t len, const int32_t* __restrict__ anchor,
                                              const uint8_t* __restrict__ type, const int32_t* __restrict__ alen,
                                              const uint8_t* __restrict__ bases, int64_t n, uint8_t* __restrict__ cls,
                                              unsigned long long* out) {
    __shared__ unsigned int s_h[ID83_BINS];
    for (int k = threadIdx.x; k < ID83_BINS; k += blockDim.x) s_h[k] = 0;
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t a = anchor[i];
        const int L = alen[i], ty = type[i];       // 1..64 and 0 / 1: the host has checked
        int bin;
        if (a < 0 || (ty == 0 ? a + L >= len : a >= len)) {
            bin = ID83_RANGE;
        } else if (ty == 0) {
            // the deleted stretch must be letters; its first is the class letter of a 1-base deletion
            bool nbase = false;
            for (int j = 0; j < L; j++) nbase |= acgt_code(seq[a + 1 + j]) > 3;
            if (nbase) {
                bin = ID83_NBASE;
            } else {
                const int cap = 5 * L;
                int r = 0, l = 0;
                while (r < cap && a + 1 + L + r < len) {
                    const int x = acgt_code(seq[a + 1 + L + r]);
                    if (x > 3 || x != acgt_code(seq[a + 1 + r])) break;
                    r++;
                }
                while (l + r < cap && a - l >= 0) {
                    const int x = acgt_code(seq[a - l]);
                    if (x > 3 || x != acgt_code(seq[a + L - l])) break;
                    l++;
                }
                bin = id83_class(0, L, acgt_code(seq[a + 1]), l + r);
            }
        } else {
            const uint4 v = *reinterpret_cast<const uint4*>(bases + i * 16);
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
            const int cap = 5 * L;
            int r = 0, l = 0, jr = 0, jl = L - 1;   // jr = r mod L, jl = (L - 1 - l) mod L
            while (r < cap && a + 1 + r < len) {
                if (acgt_code(seq[a + 1 + r]) != ins_code(w, jr)) break;
                r++;
                if (++jr == L) jr = 0;
            }
            while (l + r < cap && a - l >= 0) {
                if (acgt_code(seq[a - l]) != ins_code(w, jl)) break;
                l++;
                if (--jl < 0) jl = L - 1;
            }
            bin = id83_class(1, L, ins_code(w, 0), l + r);
        }
        atomicAdd(&s_h[bin], 1u);
        if (cls) cls[i] = (uint8_t)(bin < ID83_CLASSES ? bin : SPECTRA_NO_CLASS);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < ID83_BINS; k += blockDim.x)
        if (s_h[k]) atomicAdd(&out[k], (unsigned long long)s_h[k]);
}

// k_dbs78.  ref2 / alt2: two ASCII letters each, upper-cased here.  If the reference pair is one of the ten of the table
// the pair is taken as it is, else both are reverse-complemented; for the four self-complementary references (AT CG GC
// TA) an alternative the table does not list is replaced by its reverse complement.  The workgroup first writes the class
// of each of the 256 (reference pair, alternative pair) into LDS, then every thread looks its allele up.
__global__ void __launch_bounds__(256) k_dbs78(const uint8_t* __restrict__ ref2, const uint8_t* __restrict__ alt2, int64_t n,
                                               uint8_t* __restrict__ cls, unsigned long long* out) {
    __shared__ unsigned int s_h[DBS78_BINS];
    __shared__ uint8_t s_map[256];
    for (int k = threadIdx.x; k < DBS78_BINS; k += blockDim.x) s_h[k] = 0;
    for (int k = threadIdx.x; k < 256; k += blockDim.x) {
        int r0 = k >> 6, r1 = (k >> 4) & 3, a0 = (k >> 2) & 3, a1 = k & 3;
        int m = DBS78_UNCHANGED;
        if (r0 != a0 && r1 != a1) {
            auto find = [](int p0, int p1, int q0, int q1) {
                const char L[] = {'A', 'C', 'G', 'T'};
                for (int c = 0; c < DBS78_CLASSES; c++) {
                    const char* t = DBS78_TABLE + 4 * c;
                    if (t[0] == L[p0] && t[1] == L[p1] && t[2] == L[q0] && t[3] == L[q1]) return c;
                }
                return -1;
            };
            auto has_ref = [](int p0, int p1) {
                const char L[] = {'A', 'C', 'G', 'T'};
                for (int c = 0; c < DBS78_CLASSES; c++)
                    if (DBS78_TABLE[4 * c] == L[p0] && DBS78_TABLE[4 * c + 1] == L[p1]) return true;
                return false;
            };
            if (!has_ref(r0, r1)) {
                const int t0 = 3 - r1, t1 = 3 - r0, u0 = 3 - a1, u1 = 3 - a0;
                r0 = t0; r1 = t1; a0 = u0; a1 = u1;
            }
            int c = find(r0, r1, a0, a1);
            if (c < 0) c = find(r0, r1, 3 - a1, 3 - a0);
            m = c < 0 ? DBS78_UNCHANGED : c;       // (every pair with both bases changed has a class)
        }
        s_map[k] = (uint8_t)m;
    }
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int r0 = acgt_code(ref2[2 * i]), r1 = acgt_code(ref2[2 * i + 1]);
        const int a0 = acgt_code(alt2[2 * i]), a1 = acgt_code(alt2[2 * i + 1]);
        const int bin = (r0 | r1 | a0 | a1) > 3 ? DBS78_NLETTER : s_map[(r0 << 6) | (r1 << 4) | (a0 << 2) | a1];
        atomicAdd(&s_h[bin], 1u);
        if (cls) cls[i] = (uint8_t)(bin < DBS78_CLASSES ? bin : SPECTRA_NO_CLASS);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < DBS78_BINS; k += blockDim.x)
        if (s_h[k]) atomicAdd(&out[k], (unsigned long long)s_h[k]);
}

}  // namespace himut
