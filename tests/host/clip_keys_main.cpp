// Stand-alone driver of csrc/tld_clip_keys.h for tests/test_clip_keys_host.py: no HIP, its own main, so it also runs under AddressSanitizer + UBSan.
//   clip_keys_main <text|image> <file>      one key per line of <file> (an empty line is the empty key) -> one line each: mine | other | metadata | unknown
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>

#include "tld_clip_keys.h"

int main(int argc, char** argv) {
    if (argc != 3 || (std::strcmp(argv[1], "text") && std::strcmp(argv[1], "image"))) {
        std::fprintf(stderr, "usage: clip_keys_main <text|image> <file of keys>\n");
        return 2;
    }
    const tld::ClipTower tower = std::strcmp(argv[1], "text") ? tld::CLIP_IMAGE : tld::CLIP_TEXT;
    std::ifstream in(argv[2]);
    if (!in) { std::fprintf(stderr, "cannot read %s\n", argv[2]); return 2; }
    static const char* const kNames[] = {"mine", "other", "metadata", "unknown"};
    std::string key;
    while (std::getline(in, key)) std::printf("%s\n", kNames[tld::route_clip_key(tower, key)]);
    return 0;
}
