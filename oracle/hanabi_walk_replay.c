/*
 * TEST INFRASTRUCTURE ONLY -- replays recorded action streams through oracle/hanabi_oracle.c in a stand-alone program, so
 * that the oracle can be run under -fsanitize=address,undefined (`make sanitize-hanabi`): the evidence that the moves the
 * legal-move mask forbids (tests/hanabi_illegal_cases.py: empty hints, discards at a full pool, actions past the move
 * table and negative ones) keep the oracle inside its arrays and inside defined C.
 *
 * A stream file (written by hanabi_walk_actions.py) is int32 little-endian:
 *   colors ranks max_information_tokens max_life_tokens num_worlds num_steps, then num_steps x 2 x num_worlds actions,
 *   then one checksum (fold below, as int32 bits) of every output and record the Python-loaded oracle held after each step.
 * The replay must arrive at the same checksum: it ran the same walk.
 */
#include "mrl_oracle.h"

#include <stdio.h>
#include <stdlib.h>

/* h * 16777619 + sum of byte[i] * (i % 65521 + 1), mod 2^32: position-weighted, and cheap to restate in numpy */
static uint32_t fold(uint32_t h, const void *data, size_t bytes)
{
    const uint8_t *p = (const uint8_t *)data;
    uint64_t sum = 0;
    for (size_t i = 0; i < bytes; i++) sum += (uint64_t)p[i] * (uint64_t)(i % 65521u + 1u);
    return h * 16777619u + (uint32_t)sum;
}

static int replay(const char *path)
{
    FILE *f = fopen(path, "rb");
    if (!f) {
        fprintf(stderr, "%s: cannot open\n", path);
        return 1;
    }
    int32_t head[6];
    if (fread(head, sizeof(int32_t), 6, f) != 6 || head[4] < 1 || head[5] < 0) {
        fprintf(stderr, "%s: bad header\n", path);
        fclose(f);
        return 1;
    }
    const orc_hanabi_config cfg = {(uint32_t)head[0], (uint32_t)head[1], 2u, (uint32_t)head[2], (uint32_t)head[3]};
    const uint32_t n = (uint32_t)head[4], steps = (uint32_t)head[5];
    orc_hanabi *s = orc_hanabi_create(&cfg, n);
    int32_t *acts = (int32_t *)malloc(sizeof(int32_t) * 2 * n);
    uint8_t *records = (uint8_t *)malloc((size_t)n * orc_hanabi_record_bytes());
    if (!s || !acts || !records) {
        fprintf(stderr, "%s: configuration refused or out of memory\n", path);
        fclose(f);
        return 1;
    }
    uint32_t h = 2166136261u, finished = 0;
    int rc = 0;
    for (uint32_t t = 0; t < steps && !rc; t++) {
        if (fread(acts, sizeof(int32_t), (size_t)2 * n, f) != (size_t)2 * n) {
            fprintf(stderr, "%s: short stream at step %u\n", path, t);
            rc = 1;
            break;
        }
        orc_hanabi_step(s, acts, 1);
        orc_hanabi_dump(s, records);
        h = fold(h, orc_hanabi_obs(s), (size_t)2 * n * ORC_HANABI_OBS);
        h = fold(h, orc_hanabi_state(s), (size_t)2 * n * ORC_HANABI_STATE);
        h = fold(h, orc_hanabi_mask(s), sizeof(int32_t) * 2 * n * ORC_HANABI_MOVES);
        h = fold(h, orc_hanabi_done(s), sizeof(int32_t) * n);
        h = fold(h, records, (size_t)n * orc_hanabi_record_bytes());
        for (uint32_t w = 0; w < n; w++) finished += orc_hanabi_done(s)[w] != 0;
    }
    int32_t want = 0;
    if (!rc && fread(&want, sizeof(int32_t), 1, f) != 1) {
        fprintf(stderr, "%s: no hash at the end\n", path);
        rc = 1;
    }
    if (!rc && (uint32_t)want != h) {
        fprintf(stderr, "%s: hash %08x, the recorded walk had %08x\n", path, h, (uint32_t)want);
        rc = 1;
    }
    if (!rc)
        printf("%s: K=%u R=%u info=%u life=%u, %u worlds x %u steps, %u episodes ended, hash %08x as recorded\n", path, cfg.colors,
               cfg.ranks, cfg.max_information_tokens, cfg.max_life_tokens, n, steps, finished, h);
    free(records);
    free(acts);
    orc_hanabi_destroy(s);
    fclose(f);
    return rc;
}

int main(int argc, char **argv)
{
    if (argc < 2) {
        fprintf(stderr, "usage: %s STREAM...\n", argv[0]);
        return 2;
    }
    int rc = 0;
    for (int i = 1; i < argc; i++) rc |= replay(argv[i]);
    if (!rc) printf("hanabi_walk_replay: %d streams replayed, clean\n", argc - 1);
    return rc;
}
