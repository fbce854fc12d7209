// tts_ids -- command-line demo in the shape of the reference's test/main.cpp:75-148, built only on the public
// headers of this repo (include/SynthesizerTrn.h, include/utils.h): read a text file, load a .bin model,
// call SynthesizerTrn::infer, write a 16 kHz mono s16 WAV (44-byte RIFF header as test/main.cpp:7-65).
// Until the text frontend is wired the text file holds phoneme ids ("12 7 0 33 ...").
//
//   g++ -O2 -I include tools/cli/tts_ids.cpp -L summertts_amd/lib -lsummertts_hip -Wl,-rpath,$PWD/summertts_amd/lib -o tts_ids
//   ./tts_ids ids.txt model.bin out.wav
//   ./tts_ids --mix 3:0.6,7:0.4 ids.txt model.bin out.wav      a weighted blend of speakers (multi-speaker models, phoneme-id input; the
//                                                               reference's class has no such call: this path uses summertts_hip.h directly)
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <fstream>
#include <string>
#include <vector>

#include "SynthesizerTrn.h"
#include "summertts_hip.h"
#include "utils.h"

static void put32(char* p, uint32_t v) { memcpy(p, &v, 4); }
static void put16(char* p, uint16_t v) { memcpy(p, &v, 2); }

// RIFF/WAVE header: PCM, 1 channel, 16 kHz, 16 bit
static void wav_header(char* h, uint32_t data_bytes) {
    memcpy(h, "RIFF", 4); put32(h + 4, 36 + data_bytes); memcpy(h + 8, "WAVEfmt ", 8);
    put32(h + 16, 16); put16(h + 20, 1); put16(h + 22, 1); put32(h + 24, 16000); put32(h + 28, 16000 * 2);
    put16(h + 32, 2); put16(h + 34, 16); memcpy(h + 36, "data", 4); put32(h + 40, data_bytes);
}

static int write_wav(const char* path, const int16_t* pcm, int32_t n) {
    FILE* f = fopen(path, "wb");
    if (!f) return -1;
    char h[44];
    wav_header(h, (uint32_t)n * 2);
    fwrite(h, 44, 1, f);
    fwrite(pcm, 2, (size_t)n, f);
    fclose(f);
    return 0;
}

// "sid:weight[,sid:weight...]" -> the terms of one sts_speaker_mix
static bool parse_mix(const char* s, std::vector<int32_t>& sid, std::vector<float>& weight) {
    while (*s) {
        char* end = NULL;
        const long v = strtol(s, &end, 10);
        if (end == s || *end != ':') return false;
        s = end + 1;
        const float w = strtof(s, &end);
        if (end == s) return false;
        sid.push_back((int32_t)v); weight.push_back(w);
        s = end;
        if (*s == ',') s++;
        else if (*s) return false;
    }
    return !sid.empty();
}

// the --mix path: phoneme ids -> sts_set_speaker_mix -> sts_infer_ids
static int run_mix(const std::string& line, const char* model, const char* out, const std::vector<int32_t>& sid, const std::vector<float>& weight) {
    std::vector<int32_t> ids;
    const char* s = line.c_str();
    for (;;) {
        char* end = NULL;
        const long v = strtol(s, &end, 10);
        if (end == s) break;
        ids.push_back((int32_t)v);
        s = end;
    }
    while (*s == ' ' || *s == '\t' || *s == '\r') s++;
    if (*s || ids.empty()) { printf("--mix takes a file of phoneme ids\n"); return 2; }
    float* dataW = NULL;
    const int32_t modelSize = ttsLoadModel((char*)model, &dataW);
    if (modelSize < 0) { printf("Failed to load %s\n", model); return 1; }
    int dev = 0;
    if (const char* d = getenv("SUMMERTTS_HIP_DEVICE")) dev = atoi(d);
    sts_engine* e = NULL;
    int rc = 0;
    int16_t* pcm = NULL; int32_t n = 0;
    const sts_speaker_mix mix = {(int32_t)sid.size(), sid.data(), weight.data(), NULL, 0.f};
    if (sts_create(dataW, modelSize, dev, &e) != STS_OK || sts_set_speaker_mix(e, 1, &mix) != STS_OK ||
        sts_infer_ids(e, ids.data(), (int32_t)ids.size(), 0, 1.0f, &pcm, &n) != STS_OK) {
        printf("%s\n", sts_last_error());
        rc = 2;
    } else {
        write_wav(out, pcm, n);
        printf("%s: %d samples (%.2f s)\n", out, n, n / 16000.0);
        sts_free(pcm);
    }
    if (e) sts_destroy(e);
    tts_free_data(dataW);
    return rc;
}

int main(int argc, char** argv) {
    std::vector<int32_t> mix_sid; std::vector<float> mix_weight;
    const char* prog = argv[0];
    if (argc >= 3 && strcmp(argv[1], "--mix") == 0) {
        if (!parse_mix(argv[2], mix_sid, mix_weight)) { printf("--mix takes sid:weight[,sid:weight...]\n"); return 1; }
        argv += 2; argc -= 2;
    }
    if (argc < 4) { printf("usage: %s [--mix sid:weight[,sid:weight...]] <text-or-ids file> <model.bin> <out.wav>\n", prog); return 1; }
    std::ifstream in(argv[1]);
    if (!in) { printf("Failed to open %s\n", argv[1]); return 0; }
    std::string line, sub;
    while (std::getline(in, sub)) {
        if (sub.size() >= 3 && (unsigned char)sub[0] == 0xEF && (unsigned char)sub[1] == 0xBB && (unsigned char)sub[2] == 0xBF) sub = sub.substr(3);
        line = line + sub + "  ";      // whole file = one utterance, as the reference demo does
    }
    if (!mix_sid.empty()) return run_mix(line, argv[2], argv[3], mix_sid, mix_weight);
    float* dataW = NULL;
    int32_t modelSize = ttsLoadModel(argv[2], &dataW);
    if (modelSize < 0) { printf("Failed to load %s\n", argv[2]); return 1; }
    SynthesizerTrn* synthesizer = new SynthesizerTrn(dataW, modelSize);
    int32_t spkNum = synthesizer->getSpeakerNum();
    printf("Available speakers in the model are %d\n", spkNum);
    int rc = 0;
    if (spkNum > 20) {                 // multi-speaker demo loop of test/main.cpp:108-129
        for (int spkID = 10; spkID < 20; spkID++) {
            int32_t retLen = 0;
            int16_t* wavData = synthesizer->infer(line, spkID, 1.1, retLen);
            if (!wavData) { rc = 2; break; }
            char fileName[512];
            snprintf(fileName, sizeof(fileName), "%s_%d.wav", argv[3], spkID);
            write_wav(fileName, wavData, retLen);
            printf("%s generated\n", fileName);
            tts_free_data(wavData);
        }
    } else {
        int32_t retLen = 0;
        int16_t* wavData = synthesizer->infer(line, 0, 1.0, retLen);
        if (!wavData) rc = 2;
        else { write_wav(argv[3], wavData, retLen); printf("%s: %d samples (%.2f s)\n", argv[3], retLen, retLen / 16000.0); tts_free_data(wavData); }
    }
    delete synthesizer;
    tts_free_data(dataW);
    return rc;
}
