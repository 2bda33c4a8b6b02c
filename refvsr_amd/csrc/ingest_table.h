// The byte -> float table of the 8-bit frame formats, T[u] = (float)((double)u / 255.0): the reference loader's float64 quotient rounded
// to float32 (ingest.hip's header has the exactness argument).  One definition for every kernel that reads byte frames: ingest.hip
// (refvsr_ingest_u8) and score.hip (refvsr_score_frames); each includes it once and owns its copy in constant memory.
#pragma once

struct IngestTable { float v[256]; };
static constexpr IngestTable ingest_table() {
    IngestTable t{};
    for (int u = 0; u < 256; ++u) t.v[u] = (float)((double)u / 255.0);
    return t;
}
