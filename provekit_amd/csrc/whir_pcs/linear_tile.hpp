// linear_tile.hpp -- the register tile of the weighted-sums kernel (linear.hip): TB polynomials x TW weights per lane, one dot29
// (fe29.hpp: 17 column accumulators, one Montgomery reduction per DOT29_GROUP products) per pair.  __host__ __device__, so the CPU
// suite runs the same accumulate / flush / result code at the column bound (tools/probes: pk_probe_wsum_tile_host).
#pragma once
#include "../fe29.hpp"

namespace pkw {

template <int TB, int TW>
struct WsumTile {
    pk::dot29 d[TB][TW];
};

template <int TB, int TW>
PK_HD void wsum_tile_init(WsumTile<TB, TW>& t) {
#pragma unroll
    for (int u = 0; u < TB; u++)
#pragma unroll
        for (int v = 0; v < TW; v++) pk::dot29_init(t.d[u][v]);
}
// one element of every tiled operand: f < p, w < p (dot29's contract: the second factor travels as 32 w; a first factor of p or more
// is tolerated only now and then, see fe29.hpp -- sparse.hpp's step reduces gathered elements for that reason)
template <int TB, int TW>
PK_HD void wsum_tile_step(WsumTile<TB, TW>& t, const pk::fe (&f)[TB], const pk::fe (&w)[TW]) {
    pk::fe29 x[TB], y[TW];
#pragma unroll
    for (int u = 0; u < TB; u++) x[u] = pk::unpack29<0>(f[u]);
#pragma unroll
    for (int v = 0; v < TW; v++) y[v] = pk::unpack29<5>(w[v]);
#pragma unroll
    for (int u = 0; u < TB; u++)
#pragma unroll
        for (int v = 0; v < TW; v++) pk::dot29_add(t.d[u][v], x[u], y[v]);
}
// sum_t f_u[t] * w_v[t] * 2^-256, fully reduced
template <int TB, int TW>
PK_HD pk::fe wsum_tile_result(WsumTile<TB, TW>& t, int u, int v) {
    return pk::dot29_result(t.d[u][v]);
}

}  // namespace pkw
