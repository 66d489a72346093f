// Emission: the one pass that hands an image out of the engine (st_step, st_step_begin, the tile readers) and advances the iterate
// average (st_step, st_step_begin, st_tile_step).  emit_resolve decides, from a few facts, what that pass launches, what it books and
// what it refuses -- once, for every reader; emit.hip runs the kernel, engine_emit.cpp enqueues it.  No HIP header here:
// tests/emit_plan_host_main.cpp compiles this file alone, under the host sanitizers.
#pragma once
#include "../../include/st2.h"

namespace st2 {
// the value v of a pixel: the iterate x; the mean updated from x (mean = decay * mean + rest * x, written back) and divided by corr; a
// mean that is only read, divided by corr
enum EmitSource { EMIT_X = 0, EMIT_MEAN_UPDATED = 1, EMIT_MEAN_READ = 2 };
// the image of v: v + channel mean; (cx + channel mean) + luma(v - cx) against the content cx (st_set_original_colors)
enum EmitColour { EMIT_ADD_MEAN = 0, EMIT_LUMA = 1 };

enum EmitReader { EMIT_STEP = 0, EMIT_STEP_BEGIN, EMIT_TILE_STEP, EMIT_TILE_X, EMIT_TILE_AVERAGE, EMIT_READERS };
enum EmitContent { EMIT_CONTENT_ABSENT = 0, EMIT_CONTENT_OTHER_SIZE, EMIT_CONTENT_FITS };
enum EmitRefusal { EMIT_GRANTED = 0, EMIT_NO_CONTENT, EMIT_CONTENT_SIZE, EMIT_AVERAGE_OFF, EMIT_AVERAGE_EMPTY, EMIT_AVERAGE_BUFFER };

struct EmitFacts {
    int reader;             // EmitReader
    bool want_image;        // st_step: out_hwc given (every other reader knows by itself)
    bool averaging;         // st_set_iterate_average: decay > 0
    int avg_items;          // items in the mean so far
    bool luminance;         // st_set_original_colors
    int content;            // EmitContent: the content image against the input's size
    bool avg_fits;          // the average buffer holds 3 H W elements
};

struct EmitPlan {
    bool launch;            // false: nothing to enqueue
    int source, colour;     // EmitSource, EmitColour
    bool advance;           // items += 1 and the scalars of that item
    bool image;             // hwc is written (false: the update-only launch)
    int streams;            // 4-byte streams of the image's size that the launch moves
    bool book;              // the profiler books their bytes; false: 0 bytes -- the plain launch of st_step / st_step_begin, whose figures
                            // tests/golden/route_fingerprints.json records that way
    int status, refusal;    // ST_OK / EMIT_GRANTED, or the status and the message of the refusal: nothing may be enqueued
};

inline EmitPlan emit_refuse(int refusal)
{
    EmitPlan p{};
    p.status = ST_ERR_STATE; p.refusal = refusal;
    return p;
}

inline EmitPlan emit_resolve(const EmitFacts& f)
{
    const bool tile_reader = f.reader == EMIT_TILE_X || f.reader == EMIT_TILE_AVERAGE;
    const bool image = f.reader == EMIT_STEP ? f.want_image : f.reader != EMIT_TILE_STEP;
    if (f.reader == EMIT_TILE_AVERAGE) {
        if (!f.averaging) return emit_refuse(EMIT_AVERAGE_OFF);
        if (f.avg_items == 0) return emit_refuse(EMIT_AVERAGE_EMPTY);
    }
    const bool luma = image && f.luminance;
    if (luma && f.content != EMIT_CONTENT_FITS) return emit_refuse(f.content == EMIT_CONTENT_ABSENT ? EMIT_NO_CONTENT : EMIT_CONTENT_SIZE);
    const bool advance = !tile_reader && f.averaging;         // the tile readers read: only a step adds an item
    if (advance && !f.avg_fits) return emit_refuse(EMIT_AVERAGE_BUFFER);
    EmitPlan p{};
    p.status = ST_OK; p.refusal = EMIT_GRANTED;
    if (!image && !advance) return p;
    p.launch = true; p.image = image; p.advance = advance;
    // (an average that holds items has corr = float(1 - decay ** items) != 0 for every decay in (0, 1))
    p.source = advance ? EMIT_MEAN_UPDATED : f.reader == EMIT_TILE_AVERAGE ? EMIT_MEAN_READ : EMIT_X;
    p.colour = luma ? EMIT_LUMA : EMIT_ADD_MEAN;
    p.streams = 1;                                            // x, or the mean that is only read
    if (advance) p.streams += f.avg_items == 0 ? 1 : 2;       // the mean out, and in unless it is empty
    if (image) p.streams += luma ? 2 : 1;                     // the image out, the content in
    p.book = tile_reader || advance || luma;
    return p;
}
}  // namespace st2
