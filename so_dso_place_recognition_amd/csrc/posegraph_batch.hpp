// posegraph_batch.hpp — the batch add kernel of the closure log, compiled as part of posegraph.hip, which includes this
// file inside its anonymous namespace behind clampi() and fin().  It is a file of its own because the kernels posegraph.hip itself
// holds are counted by tests/test_reginfo_cpu.py.
#pragma once

// The batch add (pr_posegraphb_add_dev): slot p carries its own rows (i[p], j[p]) - a pose-proximity search's pair lists - and is logged
// iff accepted[p] != 0, i[p] >= 0, j[p] >= 0, i[p] != j[p], T[p] is finite and its weights (w[p], or the host pair with w == NULL) are
// finite and >= 0, in the order of p: what c calls of posegraph_add_weighted_kernel with k = 1 and query_row = j[p] leave.  One
// workgroup walks ascending chunks of 256 slots with an integer scan; thread 0 commits the count (only if some j[p] >= 0: a call of
// the single add with a negative row leaves state as it is).
__global__ __launch_bounds__(256) void posegraph_add_batch_kernel(PoseGraphView v, const int* __restrict__ di, const int* __restrict__ dj,
                                                                  const double* __restrict__ T, const unsigned char* __restrict__ accepted,
                                                                  const double* __restrict__ w, double w_rot, double w_trans, int c,
                                                                  int* __restrict__ info) {
  __shared__ int sc[256];
  if (blockIdx.x != 0) return;
  const int tid = threadIdx.x;
  const int e0 = clampi(v.state[0], v.edge_capacity);            // a scribbled count never forms an address
  int flags = v.state[1] & POSEGRAPH_OVERFLOW;
  const int room = v.edge_capacity - e0;
  int base = 0, any = 0;                                         // slots that qualify in the chunks before; some j[p] >= 0
  for (int p0 = 0; p0 < c; p0 += 256) {                          // c <= 65535: p0 + tid cannot overflow
    const int p = p0 + tid;
    bool mine = false;
    int i = -1, j = -1;
    double wr = w_rot, wt = w_trans;
    if (p < c) {
      i = di[p]; j = dj[p];
      any |= j >= 0 ? 1 : 0;
      mine = accepted[p] != 0 && i >= 0 && j >= 0 && i != j;
      for (int q = 0; q < 12; q++) mine = mine && fin(T[(size_t)p * 12 + q]);
      if (w) { wr = w[2 * (size_t)p]; wt = w[2 * (size_t)p + 1]; }
      mine = mine && fin(wr) && fin(wt) && wr >= 0.0 && wt >= 0.0;
    }
    sc[tid] = mine ? 1 : 0;
    __syncthreads();
    for (int s = 1; s < 256; s <<= 1) {
      const int x = tid >= s ? sc[tid - s] : 0;
      __syncthreads();
      sc[tid] += x;
      __syncthreads();
    }
    const int before = base + sc[tid] - (mine ? 1 : 0);
    base += sc[255];
    if (mine && before < room) {                                 // row e0 + before < edge_capacity
      const size_t e = (size_t)e0 + before;
      v.edge_ij[e * 2] = i; v.edge_ij[e * 2 + 1] = j;
      for (int q = 0; q < 12; q++) v.edge_Z[e * 12 + q] = T[(size_t)p * 12 + q];
      v.edge_w[e * 2] = wr; v.edge_w[e * 2 + 1] = wt;
    }
    __syncthreads();                                             // sc[255] has been read
  }
  any = __syncthreads_or(any);                                   // every thread has read state
  if (tid == 0) {
    const int stored = base < room ? base : room;
    if (base > room) flags |= POSEGRAPH_OVERFLOW;
    if (any) { v.state[0] = e0 + stored; v.state[1] = flags; }
    info[0] = stored; info[1] = stored > 0 ? e0 : -1; info[2] = e0 + stored; info[3] = flags;
  }
}
