// csrc/emit_plan.h on the host, alone (no HIP, no engine), under the address and undefined-behaviour sanitizers
// (tests/test_emit_plan_cpu.py builds and runs it).  One line per combination of the facts, in the order of the loops below:
//   <reader> <want> <averaging> <luminance> <content> <buffer> -> nothing | refuse <status> <message> | <source> <colour> <advance> <image> <streams> <book>
#include "../style_transfer2_amd/csrc/emit_plan.h"

#include <stdio.h>

int main()
{
    using namespace st2;
    static const char* const readers[EMIT_READERS] = {"step", "begin", "tile_step", "tile_x", "tile_average"};
    static const char* const averaging[3] = {"off", "empty", "items"};
    static const char* const contents[3] = {"absent", "other_size", "fits"};
    static const char* const refusals[] = {"granted", "no_content", "content_size", "average_off", "average_empty", "average_buffer"};
    static const char* const sources[] = {"x", "mean_updated", "mean_read"};
    static const char* const colours[] = {"add_mean", "luma"};
    int bad = 0;
    for (int reader = 0; reader < EMIT_READERS; ++reader)
        for (int want = 0; want < 2; ++want)
            for (int avg = 0; avg < 3; ++avg)
                for (int luma = 0; luma < 2; ++luma)
                    for (int content = 0; content < 3; ++content)
                        for (int fits = 0; fits < 2; ++fits) {
                            EmitFacts f{};
                            f.reader = reader; f.want_image = want != 0;
                            f.averaging = avg != 0; f.avg_items = avg == 2 ? 3 : 0;
                            f.luminance = luma != 0; f.content = content; f.avg_fits = fits != 0;
                            const EmitPlan p = emit_resolve(f);
                            printf("%s %d %s %d %s %s -> ", readers[reader], want, averaging[avg], luma, contents[content], fits ? "ok" : "bad");
                            if (p.refusal != EMIT_GRANTED) {
                                // a refused plan launches nothing and carries an error status
                                if (p.launch || p.advance || p.status == ST_OK || p.refusal < 0 || p.refusal > EMIT_AVERAGE_BUFFER) { bad++; printf("BROKEN\n"); }
                                else printf("refuse %d %s\n", p.status, refusals[p.refusal]);
                            } else if (!p.launch) {
                                if (p.status != ST_OK || p.advance || p.image || p.book) { bad++; printf("BROKEN "); }
                                printf("nothing\n");
                            } else {
                                if (p.status != ST_OK || p.source < 0 || p.source > EMIT_MEAN_READ || p.colour < 0 || p.colour > EMIT_LUMA) { bad++; printf("BROKEN\n"); continue; }
                                printf("%s %s %d %d %d %d\n", sources[p.source], colours[p.colour], p.advance ? 1 : 0, p.image ? 1 : 0, p.streams, p.book ? 1 : 0);
                            }
                        }
    return bad ? 1 : 0;
}
