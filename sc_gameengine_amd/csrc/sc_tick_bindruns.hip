// sc_tick_bindruns.hip -- what the renderer does with the sorted draw list, on the device (last piece): the bind runs of the
// list and the set of material handles the frame touched (include/sc_tick.h "bind runs").
//
// RUNS.  VkRenderer::recordCommandBuffer walks the sorted list and binds the pipeline when it changes, the material's descriptor set
// when it changes and the mesh buffers when they change (src/engine/src/sc_vk.cpp:1866-1907); a pipeline change forgets the bound
// material and mesh (boundPipeline != targetPipeline resets both).  A run is a maximal stretch of equal key (pipeline, material, mesh)
// in the first draws_sorted items; its `binds` bits are what that loop binds before the run's first draw.  The sorted keys are still in
// DrawSortState::key[] behind the sort: item t heads a run when key[t] != key[t - 1].  The run index of a head is an exclusive count of
// the heads before it: ballot + popcount inside a wave, wave totals through LDS, workgroup totals through DrawSortState::hist (free
// behind the sort).  Up to kSortGroup draws -- the reference's whole budget range -- one workgroup does all of it in one launch, like
// the radix pass; above that: head counts per workgroup, a single-workgroup scan, the rows, the counts.  A head writes every field of
// its row but `count`; `count` is the next row's `first` minus its own, written by one thread in a second step (one writer per field,
// no atomics on the table).  The table has one row more than max_runs on the device, so the last reported row finds its successor.
//
// TOUCHES.  RenderPrepStreamingSystem calls assets->touchMaterial(materialId) for every draw it emits (sc_world_partition.cpp:1322-1326),
// which marks the handle when it lies inside the table and nothing else (sc_assets.cpp:441-445): bit h is set iff an EMITTED draw -- the
// first draws_emitted entries of the visible list, behind the budget, before the renderer's filter -- has materialId == h < material_count.
// The emitted list is in visible order, not sorted: a workgroup collects its draws in an LDS bitmap (up to kTouchLdsWords words, i.e.
// 65536 material handles) and ORs its non-zero words out once; beyond that a wave ORs once per distinct word among its lanes.  The bits an
// atomicOr turns from 0 to 1 are counted: every bit of the bitmap makes that step exactly once, so the sum is materials_touched.
// Plain HIP atomics and vector stores only; every count is read on the device, every grid is fixed by capacities: the launches replay
// unchanged from a captured graph.
#include "sc_tick_internal.h"

namespace sctick {

namespace {

constexpr uint32_t kWavesPerGroup = kSortThreads / 64;           // 16
constexpr uint32_t kItemsPerWave = kSortGroup / kWavesPerGroup;  // 512 consecutive items, in index order
constexpr uint32_t kRounds = kItemsPerWave / 64;                 // 8
constexpr uint32_t kTouchLdsWords = 2048;                        // 8 KB of LDS: material tables up to 65536 handles
constexpr uint32_t kTouchItemsPerGroup = kTile * 16u;            // draws a touch workgroup is sized for

__device__ __forceinline__ uint32_t keyPipeline(uint64_t k) { return (uint32_t)(k >> 48); }
__device__ __forceinline__ uint32_t keyMaterial(uint64_t k) { return (uint32_t)(k >> 24) & 0xFFFFFFu; }
__device__ __forceinline__ uint32_t keyMesh(uint64_t k) { return (uint32_t)k & 0xFFFFFFu; }

// the reference loop's state changes between the run that ends at key `prev` and the one that starts at `key` (sc_vk.cpp:1866-1907)
__device__ __forceinline__ uint32_t bindBits(bool first, uint64_t prev, uint64_t key)
{
  if (first) return 7u;
  const uint32_t pipe = keyPipeline(prev) != keyPipeline(key) ? 1u : 0u;           // PipelineId -> VkPipeline is one to one
  const uint32_t mat = (pipe || keyMaterial(prev) != keyMaterial(key)) ? 2u : 0u;
  const uint32_t mesh = (pipe || keyMesh(prev) != keyMesh(key)) ? 4u : 0u;
  return pipe | mat | mesh;
}

__device__ __forceinline__ uint32_t waveSum(uint32_t v)
{
#pragma unroll
  for (uint32_t off = 32; off; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// heads in every workgroup's slice of the sorted list (multi-workgroup lists only)
__global__ __launch_bounds__(kSortThreads) void k_bind_head_counts(const uint64_t* __restrict__ key, const uint32_t* __restrict__ counters, uint32_t* __restrict__ groupHeads)
{
  __shared__ uint32_t waveTot[kWavesPerGroup];
  const uint32_t n = counters[kCtrDrawsSorted];
  const uint32_t base = blockIdx.x * kSortGroup;
  if (base >= n) return;                         // the scan only visits groups that hold draws
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t heads = 0;
#pragma unroll
  for (uint32_t r = 0; r < kRounds; ++r) {
    const uint32_t t = base + wave * kItemsPerWave + r * 64u + lane;
    const bool head = t < n && (t == 0u || key[t] != key[t - 1u]);
    heads += (uint32_t)__popcll(ballot64(head));
  }
  if (lane == 0) waveTot[wave] = heads;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t s = 0;
    for (uint32_t w = 0; w < kWavesPerGroup; ++w) s += waveTot[w];
    groupHeads[blockIdx.x] = s;
  }
}

// exclusive scan of the workgroups' head counts, in place, over the groups that hold draws this tick (one workgroup)
__global__ __launch_bounds__(kSortThreads) void k_bind_scan(uint32_t* groupHeads, const uint32_t* __restrict__ counters, uint32_t groups)
{
  __shared__ uint32_t waveTot[kWavesPerGroup];
  const uint32_t n = counters[kCtrDrawsSorted];
  const uint32_t active = min((n + kSortGroup - 1u) / kSortGroup, groups);
  const uint32_t per = (active + kSortThreads - 1u) / kSortThreads;
  const uint32_t b = min(threadIdx.x * per, active), e = min(b + per, active);
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t sum = 0;
  for (uint32_t i = b; i < e; ++i) sum += groupHeads[i];
  uint32_t incl = sum;
#pragma unroll
  for (uint32_t off = 1; off < 64u; off <<= 1) { const uint32_t up = __shfl_up(incl, off, 64); if (lane >= off) incl += up; }
  if (lane == 63u) waveTot[wave] = incl;
  __syncthreads();
  uint32_t run = incl - sum;
  for (uint32_t w = 0; w < wave; ++w) run += waveTot[w];
  for (uint32_t i = b; i < e; ++i) { const uint32_t v = groupHeads[i]; groupHeads[i] = run; run += v; }
}

__device__ __forceinline__ void writeCount(const BindRunState& b, uint32_t r, uint32_t runs, uint32_t n)
{
  const uint32_t next = r + 1u < runs ? b.runs[r + 1u].first : n;      // (row max_runs exists on the device for this)
  b.runs[r].count = next - b.runs[r].first;
}

// rows of this workgroup's 8192 items; kSingle: the whole list is this workgroup's, the counts and the report are written here too
template <bool kSingle>
__global__ __launch_bounds__(kSortThreads) void k_bind_rows(const uint64_t* __restrict__ key, const uint32_t* __restrict__ counters, const BindRunState b,
                                                            const uint32_t* __restrict__ groupHeads)
{
  __shared__ uint32_t waveTot[kWavesPerGroup];
  const uint32_t n = counters[kCtrDrawsSorted];
  const uint32_t base = blockIdx.x * kSortGroup;
  if (!kSingle && base >= n) return;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint64_t below = (1ull << lane) - 1ull;

  uint64_t k[kRounds], prev[kRounds], heads[kRounds];
  uint32_t inWave = 0;
#pragma unroll
  for (uint32_t r = 0; r < kRounds; ++r) {
    const uint32_t t = base + wave * kItemsPerWave + r * 64u + lane;
    k[r] = t < n ? key[t] : 0ull;
    prev[r] = (t < n && t > 0u) ? key[t - 1u] : 0ull;
    heads[r] = ballot64(t < n && (t == 0u || k[r] != prev[r]));
    inWave += (uint32_t)__popcll(heads[r]);
  }
  if (lane == 0) waveTot[wave] = inWave;
  __syncthreads();
  uint32_t run = kSingle ? 0u : groupHeads[blockIdx.x];                // heads before this wave's first item
  uint32_t groupTotal = 0;
  for (uint32_t w = 0; w < kWavesPerGroup; ++w) { const uint32_t c = waveTot[w]; if (w < wave) run += c; groupTotal += c; }

  uint32_t pipeBinds = 0, matBinds = 0, meshBinds = 0;
#pragma unroll
  for (uint32_t r = 0; r < kRounds; ++r) {
    const uint32_t t = base + wave * kItemsPerWave + r * 64u + lane;
    if ((heads[r] >> lane) & 1ull) {
      const uint32_t at = run + (uint32_t)__popcll(heads[r] & below);
      const uint32_t bits = bindBits(t == 0u, prev[r], k[r]);
      pipeBinds += bits & 1u; matBinds += (bits >> 1) & 1u; meshBinds += (bits >> 2) & 1u;
      if (at <= b.maxRuns) {                                           // row max_runs: only `first` is ever read, it is a row like the others
        BindRun24* o = &b.runs[at];
        o->first = t; o->pipeline = keyPipeline(k[r]); o->material = keyMaterial(k[r]); o->mesh = keyMesh(k[r]); o->binds = bits;
      }
    }
    run += (uint32_t)__popcll(heads[r]);
  }
  // the bind counters cover ALL runs, reported or not: reduced per wave, one atomic per wave and counter
  pipeBinds = waveSum(pipeBinds); matBinds = waveSum(matBinds); meshBinds = waveSum(meshBinds);
  if (lane == 0 && inWave) {
    if (!kSingle) atomicAdd(&b.info[kBiRuns], inWave);
    atomicAdd(&b.info[kBiPipelineBinds], pipeBinds); atomicAdd(&b.info[kBiMaterialBinds], matBinds); atomicAdd(&b.info[kBiMeshBinds], meshBinds);
  }
  if (kSingle) {
    __syncthreads();                                                   // the rows above are this workgroup's own stores: visible behind the barrier
    const uint32_t shown = min(groupTotal, b.maxRuns);
    for (uint32_t r = threadIdx.x; r < shown; r += kSortThreads) writeCount(b, r, groupTotal, n);
    if (threadIdx.x == 0) { b.info[kBiRuns] = groupTotal; b.info[kBiTruncated] = groupTotal > b.maxRuns ? 1u : 0u; b.info[kBiDraws] = n; }
  }
}

// multi-workgroup lists: the counts of the reported rows, and the report's remaining words
__global__ __launch_bounds__(kTile) void k_bind_counts(const uint32_t* __restrict__ counters, const BindRunState b)
{
  const uint32_t n = counters[kCtrDrawsSorted];
  const uint32_t runs = b.info[kBiRuns];
  const uint32_t shown = min(runs, b.maxRuns);
  for (uint32_t r = blockIdx.x * kTile + threadIdx.x; r < shown; r += gridDim.x * kTile) writeCount(b, r, runs, n);
  if (blockIdx.x == 0 && threadIdx.x == 0) { b.info[kBiTruncated] = runs > b.maxRuns ? 1u : 0u; b.info[kBiDraws] = n; }
}

// the material handles of the emitted draws
template <bool kLds>
__global__ __launch_bounds__(kTile) void k_material_touches(const DeviceState d, const BindRunState b)
{
  __shared__ uint32_t bits[kLds ? kTouchLdsWords : 1u];
  const uint32_t emitted = d.counters[4];                              // k_draw_keys left it: min(visible, budget), sc_world_partition.cpp:1306-1312
  const uint32_t lane = threadIdx.x & 63u;
  if (blockIdx.x == 0 && threadIdx.x == 0) b.info[kBiTouchWords] = b.touchWords;
  if (blockIdx.x * kTile >= emitted) return;
  uint32_t fresh = 0;                                                  // bits this lane's atomics turned from 0 to 1
  if (kLds) {
    for (uint32_t i = threadIdx.x; i < b.touchWords; i += kTile) bits[i] = 0u;
    __syncthreads();
    for (uint32_t t = blockIdx.x * kTile + threadIdx.x; t < emitted; t += gridDim.x * kTile) {
      const uint32_t h = d.materialId[d.visibleIdx[t]];
      if (h < b.materialCount) atomicOr(&bits[h >> 5], 1u << (h & 31u));          // touchMaterial: handles past the table are ignored
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < b.touchWords; i += kTile) {
      const uint32_t v = bits[i];
      if (v) fresh += (uint32_t)__popc(v & ~atomicOr(&b.touch[i], v));
    }
  } else {
    for (uint32_t base = blockIdx.x * kTile + (threadIdx.x & ~63u); base < emitted; base += gridDim.x * kTile) {      // (wave-uniform trip count)
      const uint32_t t = base + lane;
      uint32_t h = 0xFFFFFFFFu;
      if (t < emitted) h = d.materialId[d.visibleIdx[t]];
      const bool live = h < b.materialCount;
      const uint32_t word = h >> 5, bit = live ? 1u << (h & 31u) : 0u;
      uint64_t todo = ballot64(live);
      while (todo) {                                                   // one atomic per distinct word among the wave's lanes
        const uint32_t leader = (uint32_t)__ffsll((long long)todo) - 1u;
        const uint32_t w = __shfl(word, (int)leader, 64);
        const bool same = live && word == w;
        uint32_t v = same ? bit : 0u;
#pragma unroll
        for (uint32_t off = 32; off; off >>= 1) v |= __shfl_xor(v, off, 64);
        if (lane == leader) fresh += (uint32_t)__popc(v & ~atomicOr(&b.touch[w], v));
        todo &= ~ballot64(same);
      }
    }
  }
  fresh = waveSum(fresh);
  if (lane == 0 && fresh) atomicAdd(&b.info[kBiMaterialsTouched], fresh);
}

// frame read-back: report, reported rows and bitmap into the frame's block of their own (k_stage_frame's counterpart)
__global__ __launch_bounds__(kTile) void k_stage_binds(const BindRunState b, uint32_t* __restrict__ block)
{
  const uint32_t shown = min(b.info[kBiRuns], b.maxRuns);
  const uint32_t tid = blockIdx.x * kTile + threadIdx.x, stride = gridDim.x * kTile;
  if (tid < kBiWords) block[tid] = b.info[tid];
  const uint32_t* rows = reinterpret_cast<const uint32_t*>(b.runs);
  for (uint32_t i = tid; i < shown * 6u; i += stride) block[kBiWords + i] = rows[i];
  uint32_t* words = block + kBiWords + (size_t)b.maxRuns * 6u;
  for (uint32_t i = tid; i < b.touchWords; i += stride) words[i] = b.touch[i];
}

} // namespace

// behind launchSortedDraws on its stream: `sortedKeys` is the ping-pong side the last pass left the keys in, `bound` as there
void launchBindRuns(const DeviceState& d, const DrawSortState& st, const BindRunState& b, uint32_t bound, hipStream_t s)
{
  if (!b.info) return;
  hipMemsetAsync(b.info, 0, (size_t)(kBiWords + b.touchWords) * sizeof(uint32_t), s);      // (one allocation: the report, then the bitmap)
  const uint64_t* sortedKeys = st.key[st.passes & 1u];
  const uint32_t groups = std::max((bound + kSortGroup - 1) / kSortGroup, 1u);
  if (groups == 1) hipLaunchKernelGGL((k_bind_rows<true>), dim3(1), dim3(kSortThreads), 0, s, sortedKeys, d.counters, b, st.hist);
  else {
    hipLaunchKernelGGL(k_bind_head_counts, dim3(groups), dim3(kSortThreads), 0, s, sortedKeys, d.counters, st.hist);
    hipLaunchKernelGGL(k_bind_scan, dim3(1), dim3(kSortThreads), 0, s, st.hist, d.counters, groups);
    hipLaunchKernelGGL((k_bind_rows<false>), dim3(groups), dim3(kSortThreads), 0, s, sortedKeys, d.counters, b, st.hist);
    const uint32_t countBlocks = std::min(std::max((std::min(bound, b.maxRuns) + kTile - 1u) / kTile, 1u), 1024u);
    hipLaunchKernelGGL(k_bind_counts, dim3(countBlocks), dim3(kTile), 0, s, d.counters, b);
  }
  const uint32_t touchBlocks = std::min(std::max((bound + kTouchItemsPerGroup - 1u) / kTouchItemsPerGroup, 1u), 256u);
  if (b.touchWords <= kTouchLdsWords) hipLaunchKernelGGL((k_material_touches<true>), dim3(touchBlocks), dim3(kTile), 0, s, d, b);
  else hipLaunchKernelGGL((k_material_touches<false>), dim3(touchBlocks), dim3(kTile), 0, s, d, b);
}

void launchStageBinds(const BindRunState& b, uint32_t* block, hipStream_t s)
{
  const uint32_t words = kBiWords + b.maxRuns * 6u + b.touchWords;
  const uint32_t blocks = std::min(std::max((words + kTile - 1u) / kTile, 1u), 256u);
  hipLaunchKernelGGL(k_stage_binds, dim3(blocks), dim3(kTile), 0, s, b, block);
}

} // namespace sctick
