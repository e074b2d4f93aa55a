// replica_device.hip -- replica_swap_kernel launched alone on crafted arrays (tests/test_replica_kernel.py).  A program of its
// own, compiled together with mcmcpp_amd/csrc/replica.hip: launch_replica_swap, replica_shape, replica_fill_table,
// replica_slot_base and the kernel are the production lines, unchanged; what ReplicaRound (replica_round.hpp) does around them
// (table, counts, arguments) is repeated here.
//
//   replica_device CASES OUT
//
// CASES  uint64 count; per case 15 uint64 (element bytes, K, W, D, first_chain, pairs, vec_ok, byte offset of the position base,
//        logp_stride_bytes, seed, handle stream, round, byte offset of chain 0's log-posteriors in their buffer,
//        nacc_behind_logp_bytes, moved_bit), then the positions [K][W][D], the log-posterior buffer (K strides: padding and,
//        with a moved_bit, every chain's n_accept words and whatever surrounds them included) and the cross evaluations
//        [pairs][2][W], as bytes.
// OUT    per case: the positions with kGuard bytes in front and behind (two of the longest rows each, pre-filled with kPattern
//        like every byte of the allocation), the log-posterior buffer as it came, and all 15 count records (by lower chain).
//
// One launch per case, every case in this process.  A HIP error or a case the kernel must not be given ends the program at
// once with a non-zero status.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "replica_kernels.hpp"

using namespace mcmcpp;

constexpr size_t kGuard = 16384;  // two rows of 1024 doubles
constexpr int kPattern = 0xA5;

#define HIP_OR_DIE(expr)                                                                                    \
    do                                                                                                      \
    {                                                                                                       \
        const hipError_t e_ = (expr);                                                                       \
        if (e_ != hipSuccess)                                                                               \
        {                                                                                                   \
            std::fprintf(stderr, "replica_device: %s: %s (line %d)\n", #expr, hipGetErrorString(e_), __LINE__); \
            std::exit(1);                                                                                   \
        }                                                                                                   \
    } while (0)

static void refuse(size_t index, const char* why)
{
    std::fprintf(stderr, "replica_device: case %zu refused: %s\n", index, why);
    std::exit(3);
}

static void read_or_die(void* to, size_t bytes, std::FILE* f)
{
    if (bytes && std::fread(to, 1, bytes, f) != bytes)
    {
        std::fprintf(stderr, "replica_device: the case file ends early\n");
        std::exit(2);
    }
}

static void write_or_die(const void* from, size_t bytes, std::FILE* f)
{
    if (bytes && std::fwrite(from, 1, bytes, f) != bytes)
    {
        std::fprintf(stderr, "replica_device: cannot write the results\n");
        std::exit(2);
    }
}

struct Case
{
    uint64_t elem, K, W, D, first_chain, pairs, vec_ok, pos_offset, logp_stride_bytes, seed, stream, round, logp_offset, nacc_behind_logp_bytes, moved_bit;
};

template <class T>
static void run_case(size_t index, const Case& c, std::FILE* in, std::FILE* out)
{
    const int K = (int)c.K, W = (int)c.W, D = (int)c.D, pairs = (int)c.pairs, vec_ok = (int)c.vec_ok;
    const size_t pos_bytes = (size_t)K * W * D * sizeof(T), logp_bytes = (size_t)K * c.logp_stride_bytes, cross_bytes = (size_t)pairs * 2 * W * sizeof(T);
    std::vector<unsigned char> pos(pos_bytes), logp(logp_bytes), cross(cross_bytes);
    read_or_die(pos.data(), pos_bytes, in);
    read_or_die(logp.data(), logp_bytes, in);
    read_or_die(cross.data(), cross_bytes, in);

    // every byte the kernel may write lies inside these allocations, or the case is refused
    if (pairs < 1 || pairs > kReplicaMaxSlots || c.first_chain + 2 * c.pairs > c.K || c.K > 2 * kReplicaMaxSlots) refuse(index, "the pairs do not lie inside the K chains");
    if (c.logp_offset % sizeof(T) || c.logp_offset + (uint64_t)W * sizeof(T) > c.logp_stride_bytes || c.logp_stride_bytes % sizeof(T)) refuse(index, "logp_stride_bytes");
    if (c.moved_bit >> 32 || c.nacc_behind_logp_bytes % 4) refuse(index, "moved_bit");
    if (c.moved_bit && (c.nacc_behind_logp_bytes < (uint64_t)W * sizeof(T) || c.logp_offset + c.nacc_behind_logp_bytes + (uint64_t)W * 4 > c.logp_stride_bytes))
        refuse(index, "the n_accept words do not lie behind the log-posteriors inside a chain's stride");
    if (c.pos_offset >= 16 || c.pos_offset % sizeof(T)) refuse(index, "offset of the position base");
    if (c.round >= kReplicaMaxRound) refuse(index, "round");
    if (vec_ok != 0 && vec_ok != 1) refuse(index, "vec_ok");

    const size_t guarded = kGuard + pos_bytes + kGuard;
    unsigned char *d_pos_alloc = nullptr, *d_logp = nullptr, *d_cross = nullptr;
    ReplicaJump* d_table = nullptr;
    ReplicaCounts* d_counts = nullptr;
    HIP_OR_DIE(hipMalloc(&d_pos_alloc, c.pos_offset + guarded));
    HIP_OR_DIE(hipMalloc(&d_logp, logp_bytes));
    HIP_OR_DIE(hipMalloc(&d_cross, cross_bytes));
    HIP_OR_DIE(hipMemset(d_pos_alloc, kPattern, c.pos_offset + guarded));
    unsigned char* const d_base = d_pos_alloc + c.pos_offset + kGuard;
    if (vec_ok && ((uintptr_t)d_base % 16 || (size_t)D * sizeof(T) % 16)) refuse(index, "vec_ok on rows that are not aligned 16-byte pieces");
    HIP_OR_DIE(hipMemcpy(d_base, pos.data(), pos_bytes, hipMemcpyHostToDevice));
    HIP_OR_DIE(hipMemcpy(d_logp, logp.data(), logp_bytes, hipMemcpyHostToDevice));
    HIP_OR_DIE(hipMemcpy(d_cross, cross.data(), cross_bytes, hipMemcpyHostToDevice));

    // as ReplicaRound does: the stream and its table, the counts cleared, the shape, one base state per slot
    ReplicaU128 state0, inc;
    replica_seed(c.seed, c.stream, &state0, &inc);
    std::vector<ReplicaJump> t((size_t)replica_table_entries(W));
    replica_fill_table(inc, W, t.data());
    HIP_OR_DIE(hipMalloc(&d_table, sizeof(ReplicaJump) * t.size()));
    HIP_OR_DIE(hipMemcpy(d_table, t.data(), sizeof(ReplicaJump) * t.size(), hipMemcpyHostToDevice));
    HIP_OR_DIE(hipMalloc(&d_counts, sizeof(ReplicaCounts) * kReplicaCountRecords));
    HIP_OR_DIE(hipMemset(d_counts, 0, sizeof(ReplicaCounts) * kReplicaCountRecords));
    const ReplicaShape shape = replica_shape(W, D, (int)sizeof(T), vec_ok, pairs);
    if ((size_t)shape.units * shape.unit_bytes != (size_t)D * sizeof(T) || (long long)shape.grid_x * shape.walkers_per_block < W) refuse(index, "shape");
    ReplicaSwapArgs<T> a;
    std::memset(&a, 0, sizeof a);
    a.pos = reinterpret_cast<T*>(d_base), a.logp = reinterpret_cast<T*>(d_logp + c.logp_offset), a.cross = reinterpret_cast<const T*>(d_cross), a.table = d_table, a.counts = d_counts;
    a.logp_stride_bytes = c.logp_stride_bytes, a.nacc_behind_logp_bytes = c.nacc_behind_logp_bytes, a.moved_bit = (uint32_t)c.moved_bit;
    a.W = W, a.D = D, a.first_chain = (int)c.first_chain, a.lanes = shape.lanes, a.units = shape.units, a.vec_ok = vec_ok;
    for (int j = 0; j < pairs; ++j) a.base[j] = replica_slot_base(state0, inc, c.round, j, W);
    launch_replica_swap(a, shape, nullptr);
    HIP_OR_DIE(hipGetLastError());
    HIP_OR_DIE(hipDeviceSynchronize());

    std::vector<unsigned char> got_pos(guarded), got_logp(logp_bytes);
    ReplicaCounts counts[kReplicaCountRecords];
    HIP_OR_DIE(hipMemcpy(got_pos.data(), d_pos_alloc + c.pos_offset, guarded, hipMemcpyDeviceToHost));
    HIP_OR_DIE(hipMemcpy(got_logp.data(), d_logp, logp_bytes, hipMemcpyDeviceToHost));
    HIP_OR_DIE(hipMemcpy(counts, d_counts, sizeof counts, hipMemcpyDeviceToHost));
    write_or_die(got_pos.data(), guarded, out);
    write_or_die(got_logp.data(), logp_bytes, out);
    write_or_die(counts, sizeof counts, out);
    HIP_OR_DIE(hipFree(d_pos_alloc));
    HIP_OR_DIE(hipFree(d_logp));
    HIP_OR_DIE(hipFree(d_cross));
    HIP_OR_DIE(hipFree(d_table));
    HIP_OR_DIE(hipFree(d_counts));
}

int main(int argc, char** argv)
{
    static_assert(sizeof(ReplicaCounts) == 16 && kReplicaCountRecords == 15 && sizeof(Case) == 120, "the records of the two files");
    if (argc != 3) return 2;
    std::FILE* in = std::fopen(argv[1], "rb");
    std::FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out)
    {
        std::fprintf(stderr, "replica_device: cannot open %s\n", in ? argv[2] : argv[1]);
        return 2;
    }
    const auto t0 = std::chrono::steady_clock::now();
    uint64_t count = 0;
    read_or_die(&count, sizeof count, in);
    for (size_t i = 0; i < count; ++i)
    {
        Case c;
        read_or_die(&c, sizeof c, in);
        if (c.K < 2 || c.K > 16 || c.W < 1 || c.W > (1u << 20) || c.D < 1 || c.D > 1024) refuse(i, "K, W or D");
        if (c.elem == 8)
            run_case<double>(i, c, in, out);
        else if (c.elem == 4)
            run_case<float>(i, c, in, out);
        else
            refuse(i, "element bytes");
    }
    if (std::fclose(out) != 0) return 2;
    std::fclose(in);
    const double seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::printf("replica_device OK cases=%" PRIu64 " seconds=%.3f\n", count, seconds);
    return 0;
}
