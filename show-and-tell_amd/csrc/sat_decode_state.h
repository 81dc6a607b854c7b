// The LSTM stack of the stateful decode loops (sat_greedy_decode, sat_sample_decode), host only: the argument check both start
// with, and the state they step -- h / c [num_layers][B][H], initial state IN, final state OUT.  c is updated in place; a layer's h
// ping-pongs between the caller's h and its scratch h_tmp (sat_lstm_step reads one and writes the other).
#pragma once
#include "sat_internal.h"

// what both loops require of their common arguments, before anything is enqueued
inline int sat_decode_check(const float* features, const float* embed, const float* const* lstm_w, int num_layers, const float* lin_w,
                            const float* lin_b, int B, int E, int H, int V, int steps, const float* h, const float* c,
                            const float* h_tmp, const float* x_tmp, const int64_t* ids, int64_t ids_stride) {
    if (!features || !embed || !lstm_w || !lin_w || !lin_b || !h || !c || !h_tmp || !x_tmp || !ids) return SAT_ERR_ARG;
    if (B <= 0 || E <= 0 || H <= 0 || V <= 0 || num_layers < 1 || num_layers > 8 || steps < 1 || ids_stride < steps) return SAT_ERR_ARG;
    for (int i = 0; i < 4 * num_layers; ++i)
        if (!lstm_w[i]) return SAT_ERR_ARG;
    return SAT_OK;
}

struct SatDecodeStack {
    const float* const* lstm_w;       // (w_ih, w_hh, b_ih, b_hh) per layer
    float* hb[8][2];                  // per layer: the caller's h, the scratch
    int cur[8];                       // which of the two holds the live h
    float* c;
    int num_layers, B, E, H;
    sat_stream_t stream;

    SatDecodeStack(const float* const* lstm_w_, int num_layers_, int B_, int E_, int H_, float* h, float* c_, float* h_tmp,
                   sat_stream_t stream_)
        : lstm_w(lstm_w_), c(c_), num_layers(num_layers_), B(B_), E(E_), H(H_), stream(stream_) {
        for (int l = 0; l < num_layers; ++l) {
            hb[l][0] = h + (long)l * B * H;
            hb[l][1] = h_tmp + (long)l * B * H;
            cur[l] = 0;
        }
    }

    // one sat_lstm_step per layer on the input rows x [B][E]; *top = the top layer's new h
    int step(const float* x, const float** top) {
        const float* inp = x;
        for (int l = 0; l < num_layers; ++l) {
            SAT_TRY(sat_lstm_step(inp, hb[l][cur[l]], c + (long)l * B * H, lstm_w[4 * l], lstm_w[4 * l + 1], lstm_w[4 * l + 2],
                                  lstm_w[4 * l + 3], B, l == 0 ? E : H, H, hb[l][1 - cur[l]], stream));
            cur[l] = 1 - cur[l];
            inp = hb[l][cur[l]];
        }
        *top = inp;
        return SAT_OK;
    }

    // after the last step: the final h back into the caller's tensor
    int finish() {
        for (int l = 0; l < num_layers; ++l)
            if (cur[l]) {                                      // an odd number of steps: the live hidden state sits in the scratch
                hipError_t e = hipMemcpyAsync(hb[l][0], hb[l][1], (size_t)B * H * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream);
                if (e != hipSuccess) return (int)e;
            }
        return SAT_OK;
    }
};

// The same stack for teacher-forced SCORING (sat_score_captions), where the live rows of a step are a PREFIX of the R rows that
// shrinks over the steps (rows ordered by caption length, descending).  State [num_layers][R][H]; a step runs on its first `rows`
// rows only and leaves the others alone -- they are never read again.  The top layer's h is not kept here: the caller keeps every
// step's top h (the projection's operand) and hands the previous step's rows in, this step's rows out.
struct SatScoreStack {
    const float* const* lstm_w;
    float* hb[8][2];                  // layers below the top: two copies [R][H]
    int cur[8];
    float* c;
    int num_layers, R, E, H;
    sat_stream_t stream;

    SatScoreStack(const float* const* lstm_w_, int num_layers_, int R_, int E_, int H_, float* low_h /*[2][num_layers - 1][R][H]*/,
                  float* c_ /*[num_layers][R][H]*/, sat_stream_t stream_)
        : lstm_w(lstm_w_), c(c_), num_layers(num_layers_), R(R_), E(E_), H(H_), stream(stream_) {
        for (int l = 0; l + 1 < num_layers; ++l) {
            hb[l][0] = low_h + (long)l * R * H;
            hb[l][1] = low_h + (long)(num_layers - 1 + l) * R * H;
            cur[l] = 0;
        }
    }

    // where layer l < num_layers - 1 expects its initial h
    float* h_live(int l) { return hb[l][cur[l]]; }

    // one sat_lstm_step per layer on the first `rows` rows: x [rows][E]; top_in / top_out: the top layer's h before / after
    int step(const float* x, int rows, const float* top_in, float* top_out) {
        if (rows < 1 || rows > R) return SAT_ERR_ARG;
        const float* inp = x;
        for (int l = 0; l < num_layers; ++l) {
            const bool top = l == num_layers - 1;
            const float* h_in = top ? top_in : hb[l][cur[l]];
            float* h_out = top ? top_out : hb[l][1 - cur[l]];
            SAT_TRY(sat_lstm_step(inp, h_in, c + (long)l * R * H, lstm_w[4 * l], lstm_w[4 * l + 1], lstm_w[4 * l + 2], lstm_w[4 * l + 3],
                                  rows, l == 0 ? E : H, H, h_out, stream));
            if (!top) cur[l] = 1 - cur[l];
            inp = h_out;
        }
        return SAT_OK;
    }
};
