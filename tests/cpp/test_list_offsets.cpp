// The offset check of the list loader (csrc/list_offsets.h) on the host, under the address and undefined-behaviour
// sanitizers (list_offsets.mk).  Only offsets exist here: a list of 2^31 entries is two numbers.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "list_offsets.h"

static int failures = 0;

#define EXPECT(cond)                                                         \
    do {                                                                     \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } \
    } while (0)

struct Result { int rc; char msg[128]; };

static Result check(const std::vector<int64_t>& off, const char* noun, int64_t limit) {
    Result r;
    strcpy(r.msg, "(untouched)");
    r.rc = vlq::check_list_offsets(off.data(), (int64_t)off.size() - 1, noun, limit, r.msg, sizeof(r.msg));
    return r;
}

int main() {
    const int64_t two31 = int64_t(1) << 31;
    for (const char* noun : {"list_offsets", "line_offsets"}) {
        for (int64_t limit : {vlq::kIvfLenLimit, vlq::kNoLenLimit}) {
            // nlist = 1: empty and not; all lists empty
            EXPECT(check({0, 0}, noun, limit).rc == VLQ_OK);
            EXPECT(check({0, 7}, noun, limit).rc == VLQ_OK);
            EXPECT(check({0, 0, 0, 0, 0, 0}, noun, limit).rc == VLQ_OK);
            EXPECT(check({0, 3, 3, 4, 9, 9}, noun, limit).rc == VLQ_OK);
            // an accepted input leaves the message alone
            EXPECT(strcmp(check({0, 3, 3}, noun, limit).msg, "(untouched)") == 0);

            // off[0] != 0
            for (int64_t first : {int64_t(1), int64_t(-1)}) {
                const Result r = check({first, 5, 6}, noun, limit);
                EXPECT(r.rc == VLQ_ERR_INVALID);
                EXPECT(strcmp(r.msg, (std::string(noun) + "[0] != 0").c_str()) == 0);
            }

            // a drop at index 0, in the middle, at the last list: the index and the noun are in the message
            struct { std::vector<int64_t> off; int at; } drops[] = {
                {{0, -1, 4, 5, 6}, 0}, {{0, 2, 1, 5, 6}, 1}, {{0, 2, 4, 3, 6}, 2}, {{0, 2, 4, 5, 4}, 3}, {{0, -2}, 0}};
            for (const auto& c : drops) {
                const Result r = check(c.off, noun, limit);
                char want[128];
                snprintf(want, sizeof(want), "%s not monotone at %d", noun, c.at);
                EXPECT(r.rc == VLQ_ERR_INVALID);
                EXPECT(strcmp(r.msg, want) == 0);
            }

            // 2^31 - 1 entries in one list: accepted, wherever the list is
            EXPECT(check({0, two31 - 1}, noun, limit).rc == VLQ_OK);
            EXPECT(check({0, 5, 5 + two31 - 1, 5 + two31}, noun, limit).rc == VLQ_OK);
        }

        // 2^31 entries: refused where the limit is set (the first such list is named), accepted where it is not
        {
            const Result r = check({0, two31}, noun, vlq::kIvfLenLimit);
            EXPECT(r.rc == VLQ_ERR_UNSUPPORTED);
            EXPECT(strcmp(r.msg, "list 0 longer than 2^31") == 0);
        }
        {
            const Result r = check({0, 1, 1 + two31 - 1, 1 + 2 * two31 - 1, 1 + 4 * two31}, noun, vlq::kIvfLenLimit);
            EXPECT(r.rc == VLQ_ERR_UNSUPPORTED);
            EXPECT(strcmp(r.msg, "list 2 longer than 2^31") == 0);
        }
        EXPECT(check({0, two31}, noun, vlq::kNoLenLimit).rc == VLQ_OK);
        EXPECT(check({0, 1, 1 + 4 * two31}, noun, vlq::kNoLenLimit).rc == VLQ_OK);
        // a drop in front of a long list is what is reported
        EXPECT(check({0, 3, 2, 2 + two31}, noun, vlq::kIvfLenLimit).rc == VLQ_ERR_INVALID);
    }
    if (failures) { printf("%d checks failed\n", failures); return 1; }
    printf("all ok\n");
    return 0;
}
