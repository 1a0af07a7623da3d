// TEST INFRASTRUCTURE (tests/test_sanitize.py): the host side of the whole library under a sanitizer, without a GPU.
// Linked with fake_hip.cpp (device memory = zeroed host memory, kernel launches do nothing), so every device result is the
// all-zero pattern: the point at infinity / the zero digest.  What is exercised for real is everything the sanitizers can see:
//   * the device-scoped, content-addressed, reference-counted SRS registry (zk_srs_register from several threads with the same and
//     with different bytes, zk_srs_retain / zk_srs_free, eviction through zk_srs_cache_config, zk_srs_precompute under readers);
//   * threads sharing ONE zk_ctx and threads with a ctx each over one SRS -- the pattern of tests/test_concurrency_gpu.py --
//     through the host-pointer entry points (staging buffers, pinned ring, copy stream bookkeeping), blocking batches,
//     deferred rounds (begin / open_begin / reduce / end / abort, the ZK_ERR_PENDING refusals), the commitment cache (LRU list);
//   * the persistent host pool (HostPool::run from several ctxs at once) and the host tails of a round;
//   * with REAL points: zk_g1_sum_partials(_batch) -- Jacobian -> XYZZ, host additions incl. doubling and cancellation, Fermat
//     inversion, affine normalisation -- on the group generator decoded by wire.hip's own deserialiser;
//   * every allocation of one pass over the library refused in turn (section 2d: the codes returned, the ctx afterwards, what is left
//     allocated), under a fake runtime that keeps its last error until it is read, as the real one does;
//   * a residency-cache hit whose device copy is wrong, under option "cache_verify" (section 2e).
//   * the pairing (section 2f): key validation, zk_kzg_pairing_check and zk_pairing_gt against constants on both curves -- the Fq12
//     tower, the Miller loop and both final exponentiations on the host -- then one key shared by four host threads while two ctxs
//     race its first device upload, and the key freed with its device copy; the first upload is also a site of the sweep (2d).
//     Measured on the build machine: section 2f takes 0.4 s under ASan + UBSan and 0.4 s under TSan (the program prints it); the
//     sweep, now 67 sites with a BN254 key made in every pass, 9.5 s and 23.6 s of the program's 10.3 s and 25.2 s.
// Exit code 0 and "host_stress ok" = every call returned what it must; the sanitizer's own report fails the test otherwise.
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

#include "ark_plonk_amd.h"

extern "C" long fake_hip_launches();
extern "C" long fake_hip_live_allocations();
extern "C" void fake_hip_set_memory(size_t budget, size_t report_extra);
extern "C" size_t fake_hip_live_bytes();
extern "C" long fake_hip_fail_alloc_after(long k);          // the k-th allocation from now fails once (negative: off); returns what was left
extern "C" long fake_hip_flip_byte(size_t alloc_bytes);     // inverts the first byte of every live allocation of that size; returns how many
void zk_process_key_reset_for_tests(const char* path);      // csrc/hostio.hip: test hook, not part of the C ABI

#define REQUIRE(cond)                                                              \
    do {                                                                           \
        if (!(cond)) {                                                             \
            fprintf(stderr, "host_stress: %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            return 1;                                                              \
        }                                                                          \
    } while (0)

static const int CURVE = ZK_CURVE_BLS12_381;
static const size_t L = 6;      // u64 limbs of Fq

// the standard compressed encodings of the BLS12-381 G1 generator in ark-serialize's form (x little-endian, flags in the last byte):
// decoded by the library itself, so the harness needs no field arithmetic of its own
static int generator(uint64_t* xy, bool negate) {
    static const uint8_t gx_be[48] = {0x17, 0xf1, 0xd3, 0xa7, 0x31, 0x97, 0xd7, 0x94, 0x26, 0x95, 0x63, 0x8c, 0x4f, 0xa9, 0xac, 0x0f,
                                      0xc3, 0x68, 0x8c, 0x4f, 0x97, 0x74, 0xb9, 0x05, 0xa1, 0x4e, 0x3a, 0x3f, 0x17, 0x1b, 0xac, 0x58,
                                      0x6c, 0x55, 0xe8, 0x3f, 0xf9, 0x7a, 0x1a, 0xef, 0xfb, 0x3a, 0xf0, 0x0a, 0xdb, 0x22, 0xc6, 0xbb};
    uint8_t enc[48];
    for (int i = 0; i < 48; ++i) enc[i] = gx_be[47 - i];
    uint8_t inf = 0;
    // the sign bit selects one of the two points with this x; try both and keep the one asked for (y differs, x is equal)
    uint64_t a[12], b[12];
    enc[47] &= 0x3f;
    if (zk_g1_deserialize_compressed(CURVE, enc, a, &inf) != ZK_OK || inf) return 1;
    enc[47] |= 0x80;
    if (zk_g1_deserialize_compressed(CURVE, enc, b, &inf) != ZK_OK || inf) return 1;
    if (memcmp(a, b, 48) != 0 || memcmp(a + 6, b + 6, 48) == 0) return 1;
    memcpy(xy, negate ? b : a, 96);
    return 0;
}

static int real_point_arithmetic() {
    uint64_t g[12], ng[12], one[6], out[12], two_g[12], again[12];
    uint8_t inf = 0;
    REQUIRE(generator(g, false) == 0 && generator(ng, true) == 0);
    // Montgomery one of Fq: the y of GroupAffine::zero() = (0, 1), which is what an empty sum returns
    REQUIRE(zk_g1_sum_partials(CURVE, nullptr, 0, out, &inf) == ZK_OK && inf == 1);
    memcpy(one, out + 6, 48);
    auto jac = [&](const uint64_t* xy, uint64_t* p) {
        memcpy(p, xy, 96);
        memcpy(p + 12, one, 48);
    };
    uint64_t parts[4 * 18];
    jac(g, parts);
    REQUIRE(zk_g1_sum_partials(CURVE, parts, 1, out, &inf) == ZK_OK && !inf && memcmp(out, g, 96) == 0);          // G
    jac(g, parts + 18);
    REQUIRE(zk_g1_sum_partials(CURVE, parts, 2, two_g, &inf) == ZK_OK && !inf && memcmp(two_g, g, 96) != 0);      // G + G: the doubling branch
    jac(ng, parts + 18);
    REQUIRE(zk_g1_sum_partials(CURVE, parts, 2, out, &inf) == ZK_OK && inf == 1);                                 // G - G: infinity
    jac(two_g, parts);
    jac(ng, parts + 18);
    REQUIRE(zk_g1_sum_partials(CURVE, parts, 2, out, &inf) == ZK_OK && !inf && memcmp(out, g, 96) == 0);          // 2G - G = G
    // batch form: 3 ranks x 2 jobs, rank-major; job 0 = G + G - G, job 1 = 2G - G + infinity
    uint64_t batch[3 * 2 * 18];
    memset(batch, 0, sizeof batch);
    jac(g, batch + 0 * 18);
    jac(two_g, batch + 1 * 18);
    jac(g, batch + 2 * 18);
    jac(ng, batch + 3 * 18);
    jac(ng, batch + 4 * 18);
    memcpy(batch + 5 * 18, one, 48);                 // (1, 1, 0): Jacobian zero as arkworks writes it
    memcpy(batch + 5 * 18 + 6, one, 48);
    uint64_t bout[2 * 12];
    uint8_t binf[2] = {9, 9};
    REQUIRE(zk_g1_sum_partials_batch(CURVE, batch, 3, 2, bout, binf) == ZK_OK);
    REQUIRE(!binf[0] && !binf[1] && memcmp(bout, g, 96) == 0 && memcmp(bout + 12, g, 96) == 0);
    // uncompressed / compressed round trips of the results through wire.hip
    uint8_t enc[96];
    REQUIRE(zk_g1_serialize_compressed(CURVE, two_g, 0, enc) == ZK_OK);
    REQUIRE(zk_g1_deserialize_compressed(CURVE, enc, again, &inf) == ZK_OK && !inf && memcmp(again, two_g, 96) == 0);
    return 0;
}

static std::atomic<int> g_fail{0};
#define TCHECK(cond)                                                                          \
    do {                                                                                      \
        if (!(cond)) {                                                                        \
            fprintf(stderr, "host_stress thread: %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
            g_fail.fetch_add(1);                                                              \
            return;                                                                           \
        }                                                                                     \
    } while (0)

// ---- the pairing (csrc/pairing.hip): constants for sections 2d and 2f.  Montgomery limbs, made once with the package's own Python:
// H = (curves.g2x, curves.g2y) and [TAU]H = curves.g2_mul(cv, TAU) with TAU = 0x7A5C0DE of tests/conftest.py, G and TAU G = curves.g1_mul,
// each through curves.fq_to_mont; the GT values are the (1, 1) and (1, TAU) cases of tests/golden/pairing_gt.json raised to the
// library's GT_POWER (3 / 1), taken from the polynomial basis back to tower order (the inverse of pairing_ref.tower_to_poly) and
// through fq_to_mont: what zk_pairing_gt must write word for word.
static const uint64_t BLS_H[24] = {
    0xf5f28fa202940a10ull, 0xb3f5fb2687b4961aull, 0xa1a893b53e2ae580ull, 0x9894999d1a3caee9ull, 0x6f67b7631863366bull, 0x058191924350bcd7ull,
    0xa5a9c0759e23f606ull, 0xaaa0c59dbccd60c3ull, 0x3bb17e18e2867806ull, 0x1b1ab6cc8541b367ull, 0xc2b6ed0ef2158547ull, 0x11922a097360edf3ull,
    0x4c730af860494c4aull, 0x597cfa1f5e369c5aull, 0xe7e6856caa0a635aull, 0xbbefb5e96e0d495full, 0x07d3a975f0ef25a2ull, 0x0083fd8e7e80dae5ull,
    0xadc0fc92df64b05dull, 0x18aa270a2b1461dcull, 0x86adac6a3be4eba0ull, 0x79495c4ec93da33aull, 0xe7175850a43ccaedull, 0x0b2bc2a163de1bf2ull,
};
static const uint64_t BLS_TAU_H[24] = {
    0x05c4f1e50e9717aeull, 0x607304248c6a8dc0ull, 0x465890a3fdf96d60ull, 0x66aa5df2809ec30full, 0x25c282a0d0dce546ull, 0x1906ad808634f2caull,
    0x0954e3038342f9f9ull, 0xbd78334bbd518f86ull, 0x7c63d6247f8955e4ull, 0x80104760ee2bd4c5ull, 0x6009d59e286c1e32ull, 0x08280fb9ed8f78cdull,
    0x4c4389123130b04eull, 0x0b07b88733524c8cull, 0x6b02b81f410f2cceull, 0x271c0b8ba00719d0ull, 0x053bf5a3b56579d6ull, 0x1317a1d5d793d6e1ull,
    0x8ac124a68201968eull, 0xb4de75dc19c246b4ull, 0x41c5705277967080ull, 0x7892c32593f850e8ull, 0xee1ac39ebb12551bull, 0x11d357ec0f0ce730ull,
};
static const uint64_t BLS_G[12] = {
    0x5cb38790fd530c16ull, 0x7817fc679976fff5ull, 0x154f95c7143ba1c1ull, 0xf0ae6acdf3d0e747ull, 0xedce6ecc21dbf440ull, 0x120177419e0bfb75ull,
    0xbaac93d50ce72271ull, 0x8c22631a7918fd8eull, 0xdd595f13570725ceull, 0x51ac582950405194ull, 0x0e1c8c3fad0059c0ull, 0x0bbc3efc5008a26aull,
};
static const uint64_t BLS_TAU_G[12] = {
    0x1de380e05ef9e2d6ull, 0x30d4170a5d3c527cull, 0x88ecee5b18420fe6ull, 0x380111e9d2a65ef2ull, 0xc415adf69338294dull, 0x109853e2d0b38f88ull,
    0x534606a667efb488ull, 0x886d34da19d33237ull, 0x18a88105febd6527ull, 0xe3b24c58b3fc24cbull, 0xbf8ef4f639e7805bull, 0x1a010558cbf9d3b3ull,
};
static const uint64_t BLS_NEG_TAU_G[12] = {
    0x1de380e05ef9e2d6ull, 0x30d4170a5d3c527cull, 0x88ecee5b18420fe6ull, 0x380111e9d2a65ef2ull, 0xc415adf69338294dull, 0x109853e2d0b38f88ull,
    0x66b8f959980ff623ull, 0x963ecb249780cdc8ull, 0x4e88519af7f390fcull, 0x80c4ff2c3f88edf4ull, 0x8b8cb2c009642c7bull, 0x00000c916d8612e6ull,
};
static const uint64_t BLS_GT_G_H[72] = {
    0x1972e433a01f85c5ull, 0x97d32b76fd772538ull, 0xc8ce546fc96bcdf9ull, 0xcef63e7366d40614ull, 0xa611342781843780ull, 0x13f3448a3fc6d825ull,
    0xd26331b02e9d6995ull, 0x9d68a482f7797e7dull, 0x9c9b29248d39ea92ull, 0xf4801ca2e13107aaull, 0xa16c0732bdbcb066ull, 0x083ca4afba360478ull,
    0x59e261db0916b641ull, 0x2716b6f4b23e960dull, 0xc8e55b10a0bd9c45ull, 0x0bdb0bd99c4deda8ull, 0x8cf89ebf57fdaac5ull, 0x12d6b7929e777a5eull,
    0x5fc85188b0e15f35ull, 0x34a06e3a8f096365ull, 0xdb3126a6e02ad62cull, 0xfc6f5aa97d9a990bull, 0xa12f55f5eb89c210ull, 0x1723703a926f8889ull,
    0x93588f2971828778ull, 0x43f65b8611ab7585ull, 0x3183aaf5ec279fdfull, 0xfa73d7e18ac99df6ull, 0x64e176a6a64c99b0ull, 0x179fa78c58388f1full,
    0x672a0a11ca2aef12ull, 0x0d11b9b52aa3f16bull, 0xa44412d0699d056eull, 0xc01d0177221a5ba5ull, 0x66e0cede6c735529ull, 0x05f5a71e9fddc339ull,
    0xd30a88a1b062c679ull, 0x5ac56a5d35fc8304ull, 0xd0c834a6a81f290dull, 0xcd5430c2da3707c7ull, 0xf0c27ff780500af0ull, 0x09245da6e2d72eaeull,
    0x9f2e0676791b5156ull, 0xe2d1c8234918fe13ull, 0x4c9e459f3c561bf4ull, 0xa3e85e53b9d3e3c1ull, 0x820a121e21a70020ull, 0x15af618341c59accull,
    0x7c95658c24993ab1ull, 0x73eb38721ca886b9ull, 0x5256d749477434bcull, 0x8ba41902ea504a8bull, 0x04a3d3f80c86ce6dull, 0x18a64a87fb686eaaull,
    0xbb83e71bb920cf26ull, 0x2a5277ac92a73945ull, 0xfc0ee59f94f046a0ull, 0x7158cdf3786058f7ull, 0x7cc1061b82f945f6ull, 0x03f847aa9fdbe567ull,
    0x8078dba56134e657ull, 0x1cd7ec9a43998a6eull, 0xb1aa599a1a993766ull, 0xc9a0f62f0842ee44ull, 0x8e159be3b605dffaull, 0x0c86ba0d4af13fc2ull,
    0xe80ff2a06a52ffb1ull, 0x7694ca48721a906cull, 0x7583183e03b08514ull, 0xf567afdd40cee4e2ull, 0x9a6d96d2e526a5fcull, 0x197e9f49861f2242ull,
};
static const uint64_t BLS_GT_G_TAU_H[72] = {
    0xf891e6792be5d77bull, 0x5f75840872016b4dull, 0xb5beb3ef5dfde979ull, 0xac8e0c5aef0fcf2cull, 0xd91424d8750d3b24ull, 0x070308987882f269ull,
    0xd2734f20962de844ull, 0xcf74c5f49a3c1752ull, 0xb5400a62186c3ec3ull, 0xec0cd0a6454eb702ull, 0xba2f44791cbb7d1aull, 0x0d070ea7c06aed93ull,
    0xe6dfe61ea6321aacull, 0xc8ecf31261da9ab6ull, 0xb40d40b993c153d9ull, 0x4123c5f712d225ebull, 0x700d64f5a0663c07ull, 0x083aea0bdfdb21b2ull,
    0xbf99a0e987d78d53ull, 0x1046fe75a1ac0054ull, 0xd0a01cace6dd7a62ull, 0x51c260861cd2600dull, 0x05509baf6ede78a6ull, 0x006b43670629fad9ull,
    0xa422dbc538e3ff80ull, 0x911f4cc50363ac86ull, 0xf563d868f48802d0ull, 0x0e9db17ef61dfeb0ull, 0x17cb3ff164081658ull, 0x10e8dd6e22991cd2ull,
    0xd807b86ee3e820e1ull, 0xb29c6194b8dfe831ull, 0x9216553b13e6319aull, 0x299ca43a50125be9ull, 0x603f790d28b0ad27ull, 0x145e20155b1e89dcull,
    0x1b39fd1c71fcf8bdull, 0x2af93c354df1206dull, 0x650e05e27bc9f60bull, 0x66e1697aae59ed14ull, 0x85f52c113bf3aa99ull, 0x05e91b7254f6dc14ull,
    0x30db38a90c8a2f6aull, 0xdc89cb96fa12df5dull, 0xb9ad149ca57d1744ull, 0xfe7ac9db536a5380ull, 0x40793157618168e9ull, 0x0e96c22bc944d90aull,
    0x39343e3a54fb0626ull, 0x52591fdfe046db5cull, 0xfdb43d95e41ed925ull, 0x4991482c706574caull, 0x8ca92f2d1cc5d236ull, 0x0e9c4d4626d68344ull,
    0x93d19c2249ee3e00ull, 0xc92d99f9a041b749ull, 0x51df92f9b8c38c80ull, 0x6fdb1df98e8e1c4aull, 0x28e547a9175ce8efull, 0x1565f82d4467d5abull,
    0xe71b4cfe6d57d309ull, 0x88e4c97e5084219eull, 0xbc3df21f80101d6aull, 0xbcc33d500cd16669ull, 0xc19d7fedfdaa0761ull, 0x04a38448b58690f8ull,
    0x075c1d44d4072fefull, 0x96976f605dce4f83ull, 0xdd8949cc21d5cfafull, 0x8209ce42ad156857ull, 0x7a504bd0ae3cade7ull, 0x0f4a18028978404eull,
};
static const uint64_t BN_H[16] = {
    0x8e83b5d102bc2026ull, 0xdceb1935497b0172ull, 0xfbb8264797811adfull, 0x19573841af96503bull,
    0xafb4737da84c6140ull, 0x6043dd5a5802d8c4ull, 0x09e950fc52a02f86ull, 0x14fef0833aea7b6bull,
    0x619dfa9d886be9f6ull, 0xfe7fd297f59e9b78ull, 0xff9e1a62231b7dfeull, 0x28fd7eebae9e4206ull,
    0x64095b56c71856eeull, 0xdc57f922327d3cbbull, 0x55f935be33351076ull, 0x0da4a0e693fd6482ull,
};
static const uint64_t BN_TAU_H[16] = {
    0x7ef48249112bc295ull, 0xd5d8cd22462a0cefull, 0x40ce95b211add7b2ull, 0x08b88fa4fb652be7ull,
    0xbbd8ec6698df1001ull, 0x15a39b4b99a50df4ull, 0xdd724f51aac24f16ull, 0x2b3c958b169d6dd5ull,
    0x3787060df63b6a69ull, 0xe5faddef602a6d3cull, 0x48bd642ad0c99a15ull, 0x25848ee0f8fe38f3ull,
    0xa4c5f5affb9bb702ull, 0x660faf6708fa9908ull, 0x1ea00892e9c8435eull, 0x1ec6a58a8da8802eull,
};
static const uint64_t BN_G[8] = {
    0xd35d438dc58f0d9dull, 0x0a78eb28f5c70b3dull, 0x666ea36f7879462cull, 0x0e0a77c19a07df2full,
    0xa6ba871b8b1e1b3aull, 0x14f1d651eb8e167bull, 0xccdd46def0f28c58ull, 0x1c14ef83340fbe5eull,
};
static const uint64_t BN_TAU_G[8] = {
    0x8490f525a1113284ull, 0xab521dfebcb8486bull, 0x57c46a2bf913bcbbull, 0x0211e2a79da72c80ull,
    0x0390ead4c3bfd111ull, 0xab4d584de84f04d3ull, 0xeac5066271b4973dull, 0x2fe6afee0a82f178ull,
};
static const uint64_t BN_NEG_TAU_G[8] = {
    0x8490f525a1113284ull, 0xab521dfebcb8486bull, 0x57c46a2bf913bcbbull, 0x0211e2a79da72c80ull,
    0x388fa14214bd2c36ull, 0xec3412438022c5baull, 0xcd8b3f540fccc11full, 0x007d9e84d6aeaeb0ull,
};
static const uint64_t BN_GT_G_H[48] = {
    0xc556f62b2a98671dull, 0x23a59ac167bcf363ull, 0x5ef208445f5f6f37ull, 0x12adf27ccb29382aull,
    0x2e02a64acbd60549ull, 0xd618018ea58e4addull, 0x14d585f1a45ba647ull, 0x1832226987c434fcull,
    0x2306e4312363b991ull, 0x465f6072d4023bf4ull, 0xa2ff062a4a77e736ull, 0x076ea6f18435864aull,
    0x172d1f257a4d598eull, 0xddf5bc7b7ffb5ac0ull, 0xae0b22c0bbb0f602ull, 0x1b158f3c2fae9b18ull,
    0x5cf9cc917da86724ull, 0xc799dc487a0b2753ull, 0x0df2027bf1de17a7ull, 0x197cda6cc3e20636ull,
    0xf16c96d081754cdbull, 0xce0394312bceeb55ull, 0x644e4dcf1f01ff0aull, 0x0cbea85ee0b236ccull,
    0x1bb0ce0def1b82a1ull, 0x4c4c9fe1cadefa95ull, 0x746d9990cb12b27eull, 0x13495c08e5d415c5ull,
    0x9458abcb56d24998ull, 0xb17540bd2a9e5adbull, 0x9a9983c82e401a9full, 0x1614817a84c16291ull,
    0x8975b68a2bab1f9cull, 0x2fdd826b796e0f35ull, 0x6a90a35fa03dfaa5ull, 0x1ffef4581607fc37ull,
    0x7002907c28ebfe11ull, 0x7b0591d3d080da67ull, 0xde7e5aa2181f138eull, 0x210e437dfc43d951ull,
    0x988ae2485b36cf53ull, 0x5091cc0581334e54ull, 0xda7903229312ca0full, 0x2a2341538eaee95cull,
    0xd34bab373157aa84ull, 0x3511ed44fd0d8598ull, 0x67e42a0bc2ced972ull, 0x2b8f1d5dfd20c55bull,
};

// key validation, one check each way and the GT value itself on both curves: the whole tower, the Miller loop and both final
// exponentiations on the host
static int pairing_values() {
    struct Cv {
        int id;
        size_t l;
        const uint64_t *h, *tau_h, *g, *tau_g, *neg_tau_g, *gt_h, *gt_tau_h;
    };
    const Cv cvs[2] = {{ZK_CURVE_BLS12_381, 6, BLS_H, BLS_TAU_H, BLS_G, BLS_TAU_G, BLS_NEG_TAU_G, BLS_GT_G_H, BLS_GT_G_TAU_H},
                       {ZK_CURVE_BN254, 4, BN_H, BN_TAU_H, BN_G, BN_TAU_G, BN_NEG_TAU_G, BN_GT_G_H, nullptr}};
    for (const Cv& cv : cvs) {
        const size_t l = cv.l;
        void* key = nullptr;
        uint64_t pt[24];
        // off the twist: y.c0 changed in its lowest bit; unreduced: x.c0 with every bit set; either place
        memcpy(pt, cv.h, 4 * l * 8);
        pt[2 * l] ^= 1;
        REQUIRE(zk_pairing_key_new(cv.id, pt, cv.tau_h, &key) == ZK_ERR_BAD_ARG && !key);
        REQUIRE(zk_pairing_key_new(cv.id, cv.h, pt, &key) == ZK_ERR_BAD_ARG && !key);
        memcpy(pt, cv.h, 4 * l * 8);
        for (size_t i = 0; i < l; ++i) pt[i] = ~0ull;
        REQUIRE(zk_pairing_key_new(cv.id, pt, cv.tau_h, &key) == ZK_ERR_BAD_ARG && !key);
        REQUIRE(zk_pairing_key_new(cv.id, cv.h, pt, &key) == ZK_ERR_BAD_ARG && !key);
        REQUIRE(zk_pairing_key_new(cv.id, cv.h, cv.tau_h, &key) == ZK_OK && key);
        int ok = 7;
        REQUIRE(zk_kzg_pairing_check(key, cv.g, 0, cv.tau_g, 0, &ok) == ZK_OK && ok == 1);              // (G, TAU G)
        REQUIRE(zk_kzg_pairing_check(key, cv.g, 0, cv.neg_tau_g, 0, &ok) == ZK_OK && ok == 0);          // R.y negated
        REQUIRE(zk_kzg_pairing_check(key, cv.g, 1, cv.tau_g, 1, &ok) == ZK_OK && ok == 1);              // both infinity by flag
        REQUIRE(zk_kzg_pairing_check(key, cv.g, 1, cv.tau_g, 0, &ok) == ZK_OK && ok == 0);
        // an unreduced G1 coordinate is a code and leaves *ok alone
        uint64_t un[12];
        memcpy(un, cv.tau_g, 2 * l * 8);
        for (size_t i = 0; i < l; ++i) un[l + i] = ~0ull;
        ok = 7;
        REQUIRE(zk_kzg_pairing_check(key, cv.g, 0, un, 0, &ok) == ZK_ERR_BAD_ARG && ok == 7);
        uint64_t gt[72];
        REQUIRE(zk_pairing_gt(key, 0, un, 0, gt) == ZK_ERR_BAD_ARG);
        REQUIRE(zk_pairing_gt(key, 0, cv.g, 0, gt) == ZK_OK && memcmp(gt, cv.gt_h, 12 * l * 8) == 0);
        if (cv.gt_tau_h) REQUIRE(zk_pairing_gt(key, 1, cv.g, 0, gt) == ZK_OK && memcmp(gt, cv.gt_tau_h, 12 * l * 8) == 0);
        REQUIRE(zk_pairing_gt(key, 1, cv.g, 1, gt) == ZK_OK && memcmp(gt, cv.gt_h, 12 * l * 8) != 0);   // infinity: one
        zk_pairing_key_free(key);
    }
    zk_pairing_key_free(nullptr);
    return 0;
}

// several threads share ONE key on the host while two ctxs make its first device calls on the same device: the first upload is raced
// under the key's mutex (launches do nothing here; the point is the key object), then the key goes with its device copy
static int pairing_threads() {
    const long live0 = fake_hip_live_allocations();
    void* key = nullptr;
    REQUIRE(zk_pairing_key_new(ZK_CURVE_BN254, BN_H, BN_TAU_H, &key) == ZK_OK && key);
    zk_ctx* cs[2] = {nullptr, nullptr};
    void* d[2][3] = {{nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}};
    const size_t lanes = 70;
    for (int k = 0; k < 2; ++k) {
        REQUIRE(zk_ctx_create(0, &cs[k]) == ZK_OK);
        for (int j = 0; j < 3; ++j) REQUIRE(zk_dev_alloc(cs[k], lanes * 12 * 4 * 8, &d[k][j]) == ZK_OK);
    }
    const long live1 = fake_hip_live_allocations();
    std::atomic<int> go{0};
    std::vector<std::thread> th;
    for (int t = 0; t < 4; ++t)
        th.emplace_back([&, t] {
            while (!go.load()) std::this_thread::yield();
            for (int it = 0; it < 3; ++it) {
                int ok = 7;
                const bool valid = (t + it) & 1;
                TCHECK(zk_kzg_pairing_check(key, BN_G, 0, valid ? BN_TAU_G : BN_NEG_TAU_G, 0, &ok) == ZK_OK && ok == (valid ? 1 : 0));
            }
        });
    for (int k = 0; k < 2; ++k)
        th.emplace_back([&, k] {
            while (!go.load()) std::this_thread::yield();
            for (int it = 0; it < 4; ++it) {
                if ((it + k) & 1)
                    TCHECK(zk_kzg_pairing_check_batch_dev(cs[k], key, d[k][0], nullptr, d[k][1], nullptr, lanes, (uint8_t*)d[k][2]) == ZK_OK);
                else
                    TCHECK(zk_pairing_gt_batch_dev(cs[k], key, it & 1, d[k][0], nullptr, lanes, d[k][2]) == ZK_OK);
            }
        });
    go.store(1);
    for (auto& t : th) t.join();
    REQUIRE(g_fail.load() == 0);
    REQUIRE(fake_hip_live_allocations() == live1 + 1);            // ONE device copy, whichever ctx came first
    zk_pairing_key_free(key);
    REQUIRE(fake_hip_live_allocations() == live1);
    for (int k = 0; k < 2; ++k) {
        for (int j = 0; j < 3; ++j) REQUIRE(zk_dev_free(cs[k], d[k][j]) == ZK_OK);
        zk_ctx_destroy(cs[k]);
    }
    REQUIRE(fake_hip_live_allocations() == live0);
    return 0;
}

// ---- the scenario of the allocation-failure sweep (section 2d): one pass over the calls that allocate -- a ctx, an SRS and its 16-bit
// table, a blocking batch, a deferred round with an opening, the host-pointer calls behind both caches, an NTT with its plan, a circuit
// check, a lookup map, one IPA key fold and a pairing key's first device call -- at the sizes the sections above use.  Any one hipMalloc / hipHostMalloc of it may be the
// one fake_hip_fail_alloc_after() refuses.  What must hold whichever it is: every call returns ZK_OK or ZK_ERR_OOM and nothing else
// (a stale runtime error would come back as ZK_ERR_HIP or as a second ZK_ERR_OOM from a call that allocated nothing); at most ONE call
// of a pass fails, since the hook fires once and a ctx that has refused a call works again at the next; an open round can be aborted.
// A call that needs what a failed call did not deliver (the ctx, the SRS, a device buffer) is skipped.
struct Scenario {
    const std::vector<uint64_t>* srs_bytes;
    const std::vector<std::vector<uint64_t>>* polys;
    size_t n;
    int ooms = 0;           // calls of this pass that returned ZK_ERR_OOM
    int bad_line = 0;       // the first call that returned anything else, or a round that could not be aborted
    bool note(int rc, int line) {
        if (rc == ZK_ERR_OOM) ++ooms;
        else if (rc != ZK_OK && !bad_line) bad_line = line;
        return rc == ZK_OK;
    }
    // *pc: the ctx to use, created here when null (and left to the caller, who destroys it)
    void run(zk_ctx** pc) {
#define STEP(call) note((call), __LINE__)
        ooms = 0, bad_line = 0;
        if (!*pc && !STEP(zk_ctx_create(0, pc))) return;
        zk_ctx* c = *pc;
        zk_srs* s = nullptr;
        void* d[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};      // four polynomials, an output vector, a lookup map
        const size_t slots = zk_lookup_map_slots(64);
        [&] {
            if (!STEP(zk_srs_register(c, CURVE, srs_bytes->data(), nullptr, n, &s))) return;
            STEP(zk_srs_precompute(c, s));             // refused: no table, the calls below take the per-window path
            for (int k = 0; k < 6; ++k)
                if (!STEP(zk_dev_alloc(c, k == 5 ? slots * 4 : n * 32, &d[k]))) return;
            for (int k = 0; k < 4; ++k)
                if (!STEP(zk_dev_upload(c, d[k], (*polys)[k].data(), n * 32))) return;
            const void* in[4] = {d[0], d[1], d[2], d[3]};
            const uint64_t* hp[4] = {(*polys)[0].data(), (*polys)[1].data(), (*polys)[2].data(), (*polys)[3].data()};
            size_t lens[4] = {n, n, n - 1, 64};
            uint64_t xy[16 * 12], z[4] = {5, 0, 0, 0}, ch[4] = {7, 0, 0, 0};
            uint8_t inf[16];
            STEP(zk_kzg_commit_batch_dev(c, s, 4, in, lens, xy, inf));
            // a deferred round: whatever refuses, the round can be dropped and leaves nothing pending
            const bool queued = STEP(zk_kzg_round_begin_dev(c, s, 2, in, lens, nullptr)) && STEP(zk_kzg_open_begin_dev(c, s, 3, in, lens, z, ch));
            if (!queued || !STEP(zk_kzg_round_end(c, 3, xy, inf))) {
                uint32_t pend = 9;
                if ((zk_kzg_round_abort(c) != ZK_OK || zk_kzg_round_pending(c, &pend) != ZK_OK || pend != 0) && !bad_line) bad_line = __LINE__;
            }
            // the host-pointer calls with the residency and the commitment cache on
            if (STEP(zk_ctx_set_residency_cache(c, 1, 0, 0)) && STEP(zk_ctx_set_commit_cache(c, 1, 8))) {
                STEP(zk_kzg_commit_batch(c, s, 4, hp, lens, xy, inf));
                STEP(zk_kzg_open(c, s, 3, hp, lens, z, ch, xy, inf));
            }
            STEP(zk_ctx_set_residency_cache(c, 0, 0, 0));
            STEP(zk_ctx_set_commit_cache(c, 0, 0));
            STEP(zk_ntt_prepare(c, CURVE, 13));
            STEP(zk_ntt_dev(c, CURVE, ZK_NTT_IFFT, 13, d[0], n, d[4]));
            {   // a circuit check over 2^13 rows: every column is one of the vectors above (the fake device computes nothing)
                zk_circuit_check_args a;
                memset(&a, 0, sizeof a);
                a.w_l = d[0], a.w_r = d[1], a.w_o = d[2], a.w_4 = d[3];
                a.q_m = a.q_l = a.q_r = a.q_o = a.q_4 = a.q_c = a.q_arith = a.q_range = a.q_logic = a.q_fixed_group_add = a.q_variable_group_add = a.q_lookup = d[0];
                for (int k = 0; k < 4; ++k) a.sigma[k] = d[k], a.table[k] = d[k];
                a.table_rows = 64;
                zk_circuit_check_summary sum;
                STEP(zk_circuit_check_dev(c, CURVE, 13, &a, nullptr, &sum));
            }
            {   // a lookup map over the first 64 rows and 64 queries of it
                const void* ops[3] = {d[0], d[1], d[3]};
                uint64_t misses = 0, first = 0;
                if (STEP(zk_lookup_map_build_dev(c, CURVE, d[0], d[1], d[3], 64, d[5], slots)))
                    STEP(zk_lookup_map_query_dev(c, CURVE, in, 64, d[5], slots, 64, ops, nullptr, 64, d[4], nullptr, 64, nullptr, &misses, &first));
            }
            STEP(zk_ipa_fold_key_dev(c, CURVE, 64, d[0], nullptr, z, d[4], nullptr));      // 128 key points in, 64 out
            {   // a pairing key's first device call uploads its tables: refused, it leaves no device copy behind and the next call uploads
                void* key = nullptr;
                if (zk_pairing_key_new(ZK_CURVE_BN254, BN_H, BN_TAU_H, &key) != ZK_OK) {
                    if (!bad_line) bad_line = __LINE__;
                } else {
                    const long live = fake_hip_live_allocations();
                    if (!STEP(zk_kzg_pairing_check_batch_dev(c, key, d[0], nullptr, d[1], nullptr, 4, (uint8_t*)d[4]))) {
                        if (fake_hip_live_allocations() != live && !bad_line) bad_line = __LINE__;
                        if (zk_kzg_pairing_check_batch_dev(c, key, d[0], nullptr, d[1], nullptr, 4, (uint8_t*)d[4]) != ZK_OK && !bad_line) bad_line = __LINE__;
                    }
                    if (fake_hip_live_allocations() != live + 1 && !bad_line) bad_line = __LINE__;
                    STEP(zk_pairing_gt_batch_dev(c, key, 1, d[0], nullptr, 4, d[4]));      // the copy is there: nothing to allocate
                    if (fake_hip_live_allocations() != live + 1 && !bad_line) bad_line = __LINE__;
                    zk_pairing_key_free(key);
                    if (fake_hip_live_allocations() != live && !bad_line) bad_line = __LINE__;
                }
            }
        }();
        for (int k = 0; k < 6; ++k)
            if (d[k]) STEP(zk_dev_free(c, d[k]));
        if (s) zk_srs_free(s);
#undef STEP
    }
};

int main() {
    REQUIRE(real_point_arithmetic() == 0);

    const size_t n = 1 << 13;           // the smallest size that takes the window-table path (ZK_PRE_MIN_N)
    std::vector<uint64_t> srs_a(n * 2 * L), srs_b(n * 2 * L);
    for (size_t i = 0; i < srs_a.size(); ++i) {
        srs_a[i] = 0x1000 + i;          // bytes only: the fake device never looks at them, the registry digests them
        srs_b[i] = 0x9000 + 3 * i;
    }
    std::vector<std::vector<uint64_t>> polys(4, std::vector<uint64_t>(n * 4));
    for (size_t k = 0; k < polys.size(); ++k)
        for (size_t i = 0; i < polys[k].size(); ++i) polys[k][i] = (k + 1) * 1000003ull + i;

    // ---- 1. several threads register the same and different SRS bytes at once, precompute, commit through ONE shared ctx
    zk_ctx* shared = nullptr;
    REQUIRE(zk_ctx_create(0, &shared) == ZK_OK);
    {
        std::vector<std::thread> th;
        for (int t = 0; t < 6; ++t)
            th.emplace_back([&, t] {
                for (int it = 0; it < 8; ++it) {
                    zk_srs* s = nullptr;
                    TCHECK(zk_srs_register(shared, CURVE, (t & 1) ? srs_b.data() : srs_a.data(), nullptr, n, &s) == ZK_OK && s);
                    TCHECK(zk_srs_len(s) == n);
                    TCHECK(zk_srs_precompute(shared, s) == ZK_OK);
                    uint32_t c = 0, w = 0;
                    TCHECK(zk_srs_table_info(s, &c, &w) == ZK_OK && c == 16 && w == 16);
                    uint64_t xy[4 * 12];
                    uint8_t inf[4] = {0, 0, 0, 0};
                    const uint64_t* ptrs[4] = {polys[0].data(), polys[1].data(), polys[2].data(), polys[3].data()};
                    size_t lens[4] = {n, n - 1, n, 100};          // table path and a short vector (per-window path)
                    TCHECK(zk_kzg_commit_batch(shared, s, 4, ptrs, lens, xy, inf) == ZK_OK);
                    TCHECK(inf[0] && inf[1] && inf[2] && inf[3]);      // all-zero device results: the point at infinity
                    uint64_t z[4] = {5, 0, 0, 0}, ch[4] = {7, 0, 0, 0};
                    TCHECK(zk_kzg_open(shared, s, 3, ptrs, lens, z, ch, xy, inf) == ZK_OK);
                    std::vector<uint64_t> v(polys[t % 4]);
                    TCHECK(zk_ntt(shared, CURVE, ZK_NTT_IFFT, 13, v.data(), n, v.data()) == ZK_OK);
                    if (it & 1) TCHECK(zk_srs_retain(s) == ZK_OK);
                    zk_srs_free(s);
                    if (it & 1) zk_srs_free(s);
                }
            });
        for (auto& t : th) t.join();
        REQUIRE(g_fail.load() == 0);
        uint64_t hits = 0, misses = 0, entries = 0, bytes = 0;
        REQUIRE(zk_srs_cache_stats(&hits, &misses, &entries, &bytes) == ZK_OK);
        REQUIRE(misses == 2 && hits == 6 * 8 - 2 && entries == 2);
    }

    // ---- 2. a ctx per thread over ONE SRS: deferred rounds, the refusals while a round is open, abort, the commitment cache
    zk_srs* srs = nullptr;
    REQUIRE(zk_srs_register(shared, CURVE, srs_a.data(), nullptr, n, &srs) == ZK_OK);
    {
        std::vector<std::thread> th;
        for (int t = 0; t < 4; ++t)
            th.emplace_back([&, t] {
                zk_ctx* c = nullptr;
                TCHECK(zk_ctx_create(0, &c) == ZK_OK);
                std::vector<void*> d(4, nullptr);
                for (int k = 0; k < 4; ++k) {
                    TCHECK(zk_dev_alloc(c, n * 32, &d[k]) == ZK_OK);
                    TCHECK(zk_dev_upload(c, d[k], polys[k].data(), n * 32) == ZK_OK);
                }
                const void* in[4] = {d[0], d[1], d[2], d[3]};
                size_t lens[4] = {n, n, n - 1, 64};
                uint64_t xy[16 * 12];
                uint8_t inf[16];
                uint64_t z[4] = {5, 0, 0, 0}, ch[4] = {7, 0, 0, 0};
                for (int it = 0; it < 10; ++it) {
                    TCHECK(zk_kzg_round_begin_dev(c, srs, 2, in, lens, nullptr) == ZK_OK);
                    TCHECK(zk_kzg_round_begin_dev(c, srs, 2, in + 2, lens + 2, nullptr) == ZK_OK);      // a short vector joins the round
                    TCHECK(zk_kzg_open_begin_dev(c, srs, 3, in, lens, z, ch) == ZK_OK);
                    uint32_t pend = 0;
                    TCHECK(zk_kzg_round_pending(c, &pend) == ZK_OK && pend == 5);
                    TCHECK(zk_kzg_commit_dev(c, srs, d[0], n, xy, inf) == ZK_ERR_PENDING);               // blocking calls refuse
                    TCHECK(zk_kzg_round_end(c, 4, xy, inf) == ZK_ERR_BAD_ARG);                           // wrong count: stays open
                    if (it % 3 == 2) {
                        TCHECK(zk_kzg_round_abort(c) == ZK_OK);
                    } else {
                        if (it & 1) TCHECK(zk_kzg_round_reduce(c) == ZK_OK);
                        if (it & 1) TCHECK(zk_kzg_round_begin_dev(c, srs, 1, in, lens, nullptr) == ZK_ERR_PENDING);   // closed to new jobs
                        TCHECK(zk_kzg_round_end(c, 5, xy, inf) == ZK_OK);
                    }
                    TCHECK(zk_kzg_round_pending(c, &pend) == ZK_OK && pend == 0);
                    // the device form of a round's result: 2 VW sums per job on the device, summed over the ranks, combined by the host pool
                    {
                        const size_t wb = zk_winsums_dev_bytes(c, srs), pb = 256;
                        uint32_t geom[4] = {0, 0, 0, 0};
                        TCHECK(wb == 2 * 64 * pb && zk_winsums_geometry(c, srs, geom) == ZK_OK && geom[0] == 16 && geom[2] == 64);
                        void* ws = nullptr;
                        TCHECK(zk_dev_alloc(c, 2 * 4 * wb, &ws) == ZK_OK);
                        TCHECK(zk_kzg_round_begin_dev(c, srs, 4, in, lens, nullptr) == ZK_OK);
                        TCHECK(zk_kzg_round_reduce_winsums_dev(c, ws) == ZK_OK);
                        TCHECK(zk_kzg_round_end(c, 4, xy, inf) == ZK_ERR_PENDING);                // reduced towards the device: the host form refuses
                        TCHECK(zk_kzg_round_end_winsums_dev(c, 4, (char*)ws + 64) == ZK_ERR_PENDING);   // ... and so does another buffer
                        TCHECK(zk_kzg_round_end_winsums_dev(c, 4, ws) == ZK_OK);
                        TCHECK(zk_g1_sum_winsums_dev(c, srs, ws, 2, 4, xy, inf) == ZK_OK && inf[0] && inf[3]);
                        TCHECK(zk_dev_free(c, ws) == ZK_OK);
                    }
                    // tuning options: per ctx, refused while a round is open, toggled here between rounds while a second thread of the
                    // SAME ctx reads them (the ctx lock orders the two; getenv / setenv would have raced)
                    {
                        std::thread reader([&] {
                            for (int r = 0; r < 50; ++r) {
                                int64_t v = -7;
                                TCHECK(zk_ctx_get_option(c, "msm_merge", &v) == ZK_OK && (v == 0 || v == 1));
                                TCHECK(zk_ctx_get_option(c, "pre_vw", &v) == ZK_OK && (v == 0 || v == 32));
                            }
                        });
                        TCHECK(zk_ctx_set_option(c, "msm_merge", it & 1) == ZK_OK);
                        TCHECK(zk_ctx_set_option(c, "pre_vw", (it & 2) ? 32 : 0) == ZK_OK);
                        TCHECK(zk_ctx_set_option(c, "no_such_key", 1) == ZK_ERR_UNSUPPORTED && zk_ctx_set_option(c, "pre_vw", 48) == ZK_ERR_BAD_ARG);
                        TCHECK(zk_kzg_round_begin_dev(c, srs, 2, in, lens, nullptr) == ZK_OK);
                        TCHECK(zk_ctx_set_option(c, "chunk_l", 64) == ZK_ERR_PENDING);
                        TCHECK(zk_kzg_round_end(c, 2, xy, inf) == ZK_OK);
                        reader.join();
                        TCHECK(zk_ctx_set_option(c, "msm_merge", 1) == ZK_OK && zk_ctx_set_option(c, "pre_vw", 0) == ZK_OK);
                    }
                    // the residency cache of the host-pointer calls: outputs kept, inputs digested and found again, a cache of two
                    // vectors evicting under a batch of four, off = everything returned
                    {
                        const uint64_t* hp[4] = {polys[0].data(), polys[1].data(), polys[2].data(), polys[3].data()};
                        size_t hl[4] = {n, n, n - 1, 64};
                        TCHECK(zk_ctx_set_residency_cache(c, 1, (it & 1) ? 2 * n * 32 : 0, 0) == ZK_OK);
                        std::vector<uint64_t> v(polys[t % 4]);
                        TCHECK(zk_ntt(c, CURVE, ZK_NTT_IFFT, 13, v.data(), n, v.data()) == ZK_OK);          // in place: digested before it is overwritten
                        TCHECK(zk_kzg_commit_batch(c, srs, 4, hp, hl, xy, inf) == ZK_OK);
                        TCHECK(zk_kzg_commit_batch(c, srs, 4, hp, hl, xy, inf) == ZK_OK);
                        TCHECK(zk_kzg_open(c, srs, 3, hp, hl, z, ch, xy, inf) == ZK_OK);
                        uint64_t rh = 0, rm = 0, re = 0, rb = 0;
                        TCHECK(zk_residency_cache_stats(c, &rh, &rm, &re, &rb) == ZK_OK && rh >= 3 && re >= 1 && rb <= ((it & 1) ? 2 * n * 32 : ((size_t)2 << 30)));
                        TCHECK(zk_kzg_round_begin_dev(c, srs, 1, in, lens, nullptr) == ZK_OK);
                        TCHECK(zk_ctx_set_residency_cache(c, 0, 0, 0) == ZK_ERR_PENDING);
                        TCHECK(zk_kzg_round_abort(c) == ZK_OK);
                        TCHECK(zk_ctx_set_residency_cache(c, 0, 0, 0) == ZK_OK);
                        TCHECK(zk_residency_cache_stats(c, nullptr, nullptr, &re, &rb) == ZK_OK && re == 0 && rb == 0);
                    }
                    // the commitment cache: second batch is all hits
                    TCHECK(zk_ctx_set_commit_cache(c, 1, 8) == ZK_OK);
                    TCHECK(zk_kzg_commit_batch_dev(c, srs, 4, in, lens, xy, inf) == ZK_OK);
                    TCHECK(zk_kzg_commit_batch_dev(c, srs, 4, in, lens, xy, inf) == ZK_OK);
                    uint64_t h = 0, m = 0, e = 0;
                    TCHECK(zk_commit_cache_stats(c, &h, &m, &e) == ZK_OK && h >= 4 && e >= 1);
                    TCHECK(zk_ctx_set_commit_cache(c, 0, 0) == ZK_OK);
                }
                for (int k = 0; k < 4; ++k) TCHECK(zk_dev_free(c, d[k]) == ZK_OK);
                zk_ctx_destroy(c);
            });
        for (auto& t : th) t.join();
        REQUIRE(g_fail.load() == 0);
    }

    // ---- 2b. the memory budget of the deferred rounds (round 6): a begin that finds no room for another job's buffer set closes the
    // queued jobs early and reuses their sets; the option's soft limit, a "device" that really runs out (hipMalloc failing), and a
    // device too small for even one set (ZK_ERR_OOM, the ctx usable afterwards)
    {
        std::vector<void*> d(4, nullptr);
        zk_ctx* c = nullptr;
        REQUIRE(zk_ctx_create(0, &c) == ZK_OK);
        for (int k = 0; k < 4; ++k) {
            REQUIRE(zk_dev_alloc(c, n * 32, &d[k]) == ZK_OK);
            REQUIRE(zk_dev_upload(c, d[k], polys[k].data(), n * 32) == ZK_OK);
        }
        const void* in[8] = {d[0], d[1], d[2], d[3], d[0], d[1], d[2], d[3]};
        size_t lens[8] = {n, n, n - 1, 64, n, n - 2, n, n};
        uint64_t xy[16 * 12], z[4] = {5, 0, 0, 0}, ch[4] = {7, 0, 0, 0};
        uint8_t inf[16];
        uint64_t closes = 0, set_bytes = 0, fr = 0, tot = 0;
        REQUIRE(zk_ctx_set_option(c, "round_mem_limit_mb", 40) == ZK_OK && zk_ctx_set_option(c, "mem_reserve_mb", 0) == ZK_OK);
        for (int it = 0; it < 3; ++it) {
            REQUIRE(zk_kzg_round_begin_dev(c, srs, 8, in, lens, nullptr) == ZK_OK);
            REQUIRE(zk_kzg_open_begin_dev(c, srs, 3, in, lens, z, ch) == ZK_OK);
            REQUIRE(zk_kzg_round_begin_dev(c, srs, 4, in, lens, nullptr) == ZK_OK);
            if (it == 1) REQUIRE(zk_kzg_round_reduce(c) == ZK_OK);
            REQUIRE(zk_kzg_round_end(c, 13, xy, inf) == ZK_OK && inf[0] && inf[12]);
        }
        REQUIRE(zk_round_mem_stats(c, &closes, &set_bytes, &fr, &tot) == ZK_OK && closes >= 3 && set_bytes < ((size_t)110 << 20) && tot > fr);     // two table-path sets of 19 MB (nine without the
                                                                                          // budget); n - 1, n - 2 and 64 are per-window jobs
        REQUIRE(zk_kzg_commit_batch_dev(c, srs, 8, in, lens, xy, inf) == ZK_OK && inf[7]);       // the blocking batch in pieces
        REQUIRE(zk_ctx_set_option(c, "round_mem_limit_mb", 0) == ZK_OK);
        zk_ctx_destroy(c);
        // a device with room for about three sets beyond what is live: hipMemGetInfo says so first, hipMalloc itself when the reserve hides it
        for (int lie = 0; lie < 2; ++lie) {
            REQUIRE(zk_ctx_create(0, &c) == ZK_OK);
            REQUIRE(zk_ctx_set_option(c, "mem_reserve_mb", 0) == ZK_OK);
            fake_hip_set_memory(fake_hip_live_bytes() + ((size_t)56 << 20), lie ? (size_t)1 << 30 : 0);
            REQUIRE(zk_kzg_round_begin_dev(c, srs, 8, in, lens, nullptr) == ZK_OK);
            REQUIRE(zk_kzg_open_begin_dev(c, srs, 3, in, lens, z, ch) == ZK_OK);
            REQUIRE(zk_kzg_round_end(c, 9, xy, inf) == ZK_OK && inf[8]);
            REQUIRE(zk_round_mem_stats(c, &closes, nullptr, &fr, nullptr) == ZK_OK && closes >= 1 && (lie || fr < ((size_t)56 << 20)));
            // too small for a single set: ZK_ERR_OOM, nothing queued, the round can be dropped and the ctx works again with memory back
            fake_hip_set_memory(fake_hip_live_bytes() + ((size_t)1 << 20), 0);
            zk_ctx* c2 = nullptr;
            REQUIRE(zk_ctx_create(0, &c2) == ZK_OK);
            REQUIRE(zk_kzg_round_begin_dev(c2, srs, 2, in, lens, nullptr) == ZK_ERR_OOM);
            REQUIRE(zk_kzg_round_abort(c2) == ZK_OK);
            REQUIRE(zk_kzg_commit_batch_dev(c2, srs, 2, in, lens, xy, inf) == ZK_ERR_OOM);
            fake_hip_set_memory(0, 0);
            REQUIRE(zk_kzg_commit_batch_dev(c2, srs, 2, in, lens, xy, inf) == ZK_OK && inf[1]);
            zk_ctx_destroy(c2);
            zk_ctx_destroy(c);
        }
        REQUIRE(zk_ctx_create(0, &c) == ZK_OK);
        for (int k = 0; k < 4; ++k) REQUIRE(zk_dev_free(c, d[k]) == ZK_OK);
        zk_ctx_destroy(c);
    }

    // ---- 2c. the caches' error paths and guarantees (round 6)
    {
        zk_ctx* c = nullptr;
        REQUIRE(zk_ctx_create(0, &c) == ZK_OK);
        const uint64_t* hp[4] = {polys[0].data(), polys[1].data(), polys[2].data(), polys[3].data()};
        size_t hl[4] = {n, n, n - 1, 64};
        uint64_t xy[16 * 12], z[4] = {5, 0, 0, 0}, ch[4] = {7, 0, 0, 0};
        uint8_t inf[16];
        uint64_t h0 = 0, m0 = 0, e0 = 0, b0 = 0, h1 = 0, m1 = 0, e1 = 0, b1 = 0;
        REQUIRE(zk_ctx_set_residency_cache(c, 1, 0, 0) == ZK_OK);
        REQUIRE(zk_kzg_commit_batch(c, srs, 2, hp, hl, xy, inf) == ZK_OK);                 // two vectors resident
        REQUIRE(zk_residency_cache_stats(c, &h0, &m0, &e0, &b0) == ZK_OK && e0 == 2);
        // a call that fails AFTER it has created entries (a staging buffer of a later polynomial finds no memory): the entries it made or
        // touched are gone -- their digests would name bytes that never arrived -- and the same call succeeds once memory is back
        fake_hip_set_memory(fake_hip_live_bytes() + 4096, 0);
        REQUIRE(zk_kzg_open(c, srs, 4, hp, hl, z, ch, xy, inf) == ZK_ERR_OOM);
        REQUIRE(zk_residency_cache_stats(c, &h1, &m1, &e1, &b1) == ZK_OK && e1 <= e0 && b1 <= b0);
        REQUIRE(zk_ctx_set_commit_cache(c, 1, 8) == ZK_OK);
        zk_ctx* cfresh = nullptr;                                                       // no staging buffers yet: its first upload fails
        REQUIRE(zk_ctx_create(0, &cfresh) == ZK_OK);
        REQUIRE(zk_ctx_set_residency_cache(cfresh, 1, 0, 0) == ZK_OK && zk_ctx_set_commit_cache(cfresh, 1, 8) == ZK_OK);
        REQUIRE(zk_kzg_commit_batch(cfresh, srs, 4, hp, hl, xy, inf) == ZK_ERR_OOM);
        REQUIRE(zk_residency_cache_stats(cfresh, nullptr, nullptr, &e1, &b1) == ZK_OK && e1 == 0 && b1 == 0);
        fake_hip_set_memory(0, 0);
        REQUIRE(zk_kzg_commit_batch(cfresh, srs, 4, hp, hl, xy, inf) == ZK_OK && inf[0] && inf[3]);
        REQUIRE(zk_kzg_open(c, srs, 4, hp, hl, z, ch, xy, inf) == ZK_OK);
        zk_ctx_destroy(cfresh);
        // cache_verify: every hit is checked against the real thing; nothing may be found wrong
        uint64_t checked = 0, wrong = 9;
        REQUIRE(zk_ctx_set_option(c, "cache_verify", 1) == ZK_OK);
        REQUIRE(zk_kzg_commit_batch(c, srs, 4, hp, hl, xy, inf) == ZK_OK);
        REQUIRE(zk_kzg_commit_batch(c, srs, 4, hp, hl, xy, inf) == ZK_OK);
        REQUIRE(zk_kzg_open(c, srs, 3, hp, hl, z, ch, xy, inf) == ZK_OK);
        REQUIRE(zk_cache_verify_stats(c, &checked, &wrong) == ZK_OK && checked >= 6 && wrong == 0);
        REQUIRE(zk_ctx_set_option(c, "cache_verify", 0) == ZK_OK && zk_ctx_set_option(c, "cache_verify", 2) == ZK_ERR_BAD_ARG);
        zk_ctx_destroy(c);
        // no operating-system entropy behind the digest key: the caches whose hits replace a computation refuse to switch on, and the
        // SRS registry shares nothing
        zk_process_key_reset_for_tests("/nonexistent/entropy");
        REQUIRE(zk_ctx_create(0, &c) == ZK_OK);
        REQUIRE(zk_ctx_set_commit_cache(c, 1, 8) == ZK_ERR_UNSUPPORTED && zk_ctx_set_residency_cache(c, 1, 0, 0) == ZK_ERR_UNSUPPORTED);
        REQUIRE(zk_ctx_set_commit_cache(c, 0, 0) == ZK_OK && zk_ctx_set_residency_cache(c, 0, 0, 0) == ZK_OK);
        zk_srs *s1 = nullptr, *s2 = nullptr;
        REQUIRE(zk_srs_register(c, CURVE, srs_a.data(), nullptr, n, &s1) == ZK_OK && zk_srs_register(c, CURVE, srs_a.data(), nullptr, n, &s2) == ZK_OK);
        REQUIRE(s1 != s2 && s1 != srs);
        REQUIRE(zk_kzg_commit_batch(c, s1, 2, hp, hl, xy, inf) == ZK_OK);
        zk_srs_free(s1);
        zk_srs_free(s2);
        zk_ctx_destroy(c);
        zk_process_key_reset_for_tests(nullptr);
    }

    // ---- 2d. the allocation-failure sweep: the scenario above with its k-th allocation refused, for every k it has
    {
        std::vector<uint64_t> srs_c(n * 2 * L);
        for (size_t i = 0; i < srs_c.size(); ++i) srs_c[i] = 0x5000 + 7 * i;      // bytes no other section registers
        REQUIRE(zk_srs_cache_config(0) == ZK_OK && zk_srs_cache_config((size_t)32 << 30) == ZK_OK);      // idle entries of the sections above
        const auto t0 = std::chrono::steady_clock::now();
        const long live0 = fake_hip_live_allocations(), far = 1l << 40;
        Scenario sc{&srs_c, &polys, n};
        // one pass of the scenario on *pc (created when null), then the ctx destroyed and the SRS evicted: nothing of the pass is left
        auto pass = [&](zk_ctx** pc, bool keep_ctx) {
            sc.run(pc);
            if (!keep_ctx && *pc) {
                zk_ctx_destroy(*pc);
                *pc = nullptr;
            }
            return zk_srs_cache_config(0) == ZK_OK && zk_srs_cache_config((size_t)32 << 30) == ZK_OK && sc.bad_line == 0;
        };
        zk_ctx* c = nullptr;
        fake_hip_fail_alloc_after(far);                              // counts, never fires
        REQUIRE(pass(&c, false) && sc.ooms == 0);
        const long counted = far - fake_hip_fail_alloc_after(-1);
        REQUIRE(counted > 20 && fake_hip_live_allocations() == live0);
        long swept = 0;
        for (long k = 0;; ++k) {
            fake_hip_fail_alloc_after(k);
            const bool ok = pass(&c, true);
            const bool fired = fake_hip_fail_alloc_after(-1) < 0;
            if (!ok || sc.ooms > 1 || (!fired && sc.ooms)) {
                fprintf(stderr, "host_stress: allocation %ld refused: host_stress.cpp:%d returned neither ZK_OK nor ZK_ERR_OOM, or %d calls failed\n", k,
                        sc.bad_line, sc.ooms);
                return 1;
            }
            if (fired) {
                ++swept;
                if (c) REQUIRE(pass(&c, false) && sc.ooms == 0);      // the ctx that met the refusal: everything works
            } else if (c) {
                zk_ctx_destroy(c);
                c = nullptr;
            }
            REQUIRE(fake_hip_live_allocations() == live0);
            if (!fired) break;                                        // the scenario has no k-th allocation: every one was refused once
            REQUIRE(pass(&c, false) && sc.ooms == 0);                 // ... and so does a fresh one
            REQUIRE(fake_hip_live_allocations() == live0);
        }
        REQUIRE(swept >= counted);                                    // a scenario that shrank under injection would pass with fewer
        printf("host_stress: allocation sweep: %ld allocation sites refused one by one (%ld counted without injection), %.1f s\n", swept, counted,
               std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    }

    // ---- 2f. the pairing: values on both curves; one key shared by host threads while two ctxs race its first upload
    {
        const auto t0 = std::chrono::steady_clock::now();
        REQUIRE(pairing_values() == 0);
        const auto t1 = std::chrono::steady_clock::now();
        REQUIRE(pairing_threads() == 0);
        printf("host_stress: pairing: values %.1f s, threads %.1f s\n", std::chrono::duration<double>(t1 - t0).count(),
               std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count());
    }

    // ---- 2e. cache_verify meets a wrong hit: the resident copy of a vector no longer holds what its digest names
    {
        zk_ctx* c = nullptr;
        REQUIRE(zk_ctx_create(0, &c) == ZK_OK);
        REQUIRE(zk_ctx_set_residency_cache(c, 1, 0, 0) == ZK_OK && zk_ctx_set_option(c, "cache_verify", 1) == ZK_OK);
        const size_t m = n - 5, bytes = m * 32;                       // a length no other vector of the program has
        const size_t alloc = bytes + bytes / 8 + 256;                 // what a device buffer of `bytes` allocates (DevBuf::want_for, csrc/ctx.h)
        const uint64_t* hp[3] = {polys[3].data(), polys[3].data(), polys[0].data()};
        size_t hl[3] = {m, m, n};
        uint64_t xy[3 * 12];
        uint8_t inf[3];
        REQUIRE(zk_kzg_commit_batch(c, srs, 3, hp, hl, xy, inf) == ZK_OK);              // both vectors resident
        uint64_t h0 = 0, m0 = 0, e0 = 0, b0 = 0, h1 = 0, m1 = 0, e1 = 0, b1 = 0, chk0 = 0, bad0 = 9, chk1 = 0, bad1 = 9;
        REQUIRE(zk_residency_cache_stats(c, &h0, &m0, &e0, &b0) == ZK_OK && e0 == 2 && b0 == bytes + n * 32);
        REQUIRE(zk_cache_verify_stats(c, &chk0, &bad0) == ZK_OK && bad0 == 0);
        const long live = fake_hip_live_allocations();
        REQUIRE(fake_hip_flip_byte(alloc) >= 1);                      // the device copy (and the ctx's scratch buffers of that length, which
                                                                      // nothing reads on the fake device): the one mismatch below is the proof
        // the vector twice in one batch, and the other one: the first finds the entry wrong and replaces it, the second uses the replacement
        REQUIRE(zk_kzg_commit_batch(c, srs, 3, hp, hl, xy, inf) == ZK_OK && inf[0] && inf[2]);
        REQUIRE(zk_cache_verify_stats(c, &chk1, &bad1) == ZK_OK && bad1 == bad0 + 1 && chk1 == chk0 + 2);
        REQUIRE(zk_residency_cache_stats(c, &h1, &m1, &e1, &b1) == ZK_OK && e1 == e0 && b1 == b0 && h1 == h0 + 2 && m1 == m0 + 1);
        REQUIRE(fake_hip_live_allocations() == live);                 // the dropped entry's buffer took the upload
        REQUIRE(zk_kzg_commit_batch(c, srs, 3, hp, hl, xy, inf) == ZK_OK);              // again: three hits, all checked, nothing wrong
        REQUIRE(zk_cache_verify_stats(c, &chk0, &bad0) == ZK_OK && bad0 == bad1 && chk0 == chk1 + 3);
        REQUIRE(zk_residency_cache_stats(c, &h0, &m0, &e0, &b0) == ZK_OK && e0 == e1 && b0 == b1 && h0 == h1 + 3 && m0 == m1);
        zk_ctx_destroy(c);
    }

    // ---- 3. eviction: drop every unreferenced entry, then the last references
    zk_srs_free(srs);
    REQUIRE(zk_srs_cache_config(0) == ZK_OK);
    uint64_t entries = 99;
    REQUIRE(zk_srs_cache_stats(nullptr, nullptr, &entries, nullptr) == ZK_OK && entries == 0);
    REQUIRE(zk_srs_cache_config((size_t)32 << 30) == ZK_OK);
    zk_ctx_destroy(shared);
    REQUIRE(fake_hip_launches() > 1000);
    REQUIRE(fake_hip_live_allocations() == 0);        // every device / pinned buffer of every ctx and SRS was returned
    printf("host_stress ok: %ld kernel launches (no-ops), all device memory returned\n", fake_hip_launches());
    return 0;
}
