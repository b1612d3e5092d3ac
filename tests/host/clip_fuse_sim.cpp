// The host decisions of the two-launch clipped PPO step (fsrl_amd/csrc/host_decisions.hpp) as a plain program: the selection rule of
// an update and of a step, the replay decision and what a replay starts from.  Prints one "ok <name>" line per group of cases and
// exits non-zero at the first case that fails (tests/test_clip_fuse_host.py).
#include <cstdio>
#include <cstdlib>
#include "host_decisions.hpp"

static int checks = 0;
#define EXPECT(cond) do { ++checks; if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

// the headline context: solo fused PPO-Lagrangian, clip 0.5, hidden 256 with three networks (244 blocks) on 256 CUs
static ClipFuseFacts headline() {
    ClipFuseFacts f{};
    f.mode = -1; f.env_off = false; f.dead = false;
    f.ppo_lag = true; f.layered = false; f.grouped = false;
    f.recompute_adv = false; f.rew_norm = false;
    f.max_grad_norm = 0.5f; f.nparts = 244; f.n_cus = 256; f.obs_dim = 60; f.live_contexts = 1;
    return f;
}

int main() {
    {   // ---- the update rule: every condition on its own
        ClipFuseFacts f = headline();
        EXPECT(clip_fuse_update_ok(f));
        f.mode = 1; EXPECT(clip_fuse_update_ok(f));
        f.mode = 0; EXPECT(!clip_fuse_update_ok(f));
        f = headline(); f.env_off = true; EXPECT(!clip_fuse_update_ok(f));
        f.mode = 1; EXPECT(!clip_fuse_update_ok(f));                       // the environment switch beats the setter
        f = headline(); f.dead = true; f.mode = 1; EXPECT(!clip_fuse_update_ok(f));   // after a fallback: off for good
        f = headline(); f.ppo_lag = false; EXPECT(!clip_fuse_update_ok(f));
        f = headline(); f.layered = true; EXPECT(!clip_fuse_update_ok(f));
        f = headline(); f.grouped = true; EXPECT(!clip_fuse_update_ok(f));
        f = headline(); f.recompute_adv = true; EXPECT(!clip_fuse_update_ok(f));
        f = headline(); f.rew_norm = true; EXPECT(!clip_fuse_update_ok(f));
        f = headline(); f.max_grad_norm = 0.0f; EXPECT(!clip_fuse_update_ok(f));      // no clip: nothing to exchange
        f = headline(); f.max_grad_norm = -1.0f; EXPECT(!clip_fuse_update_ok(f));
        f = headline(); f.mode = 1; f.recompute_adv = true; EXPECT(!clip_fuse_update_ok(f));   // "on" forces nothing a replay cannot redo
        f = headline(); f.live_contexts = 3; EXPECT(!clip_fuse_update_ok(f));         // automatic: only a context alone on its device
        f.mode = 1; EXPECT(clip_fuse_update_ok(f));                                   // the setter may still ask for it
        printf("ok update_rule\n");
    }
    {   // ---- residency: every block of the launch on a CU of its own
        ClipFuseFacts f = headline();
        f.nparts = 256; EXPECT(clip_fuse_update_ok(f));
        f.nparts = 257; EXPECT(!clip_fuse_update_ok(f));
        f.n_cus = 304; EXPECT(clip_fuse_update_ok(f));
        f.nparts = 244; f.n_cus = 243; EXPECT(!clip_fuse_update_ok(f));
        f.nparts = 1025; f.n_cus = 2048; EXPECT(!clip_fuse_update_ok(f));            // one poller thread per block, 1 024 threads
        f.nparts = 1024; EXPECT(clip_fuse_update_ok(f));
        f = headline(); f.nparts = 325; f.n_cus = 256; EXPECT(!clip_fuse_update_ok(f));   // four networks at hidden 256
        f = headline(); f.obs_dim = CLIP_FUSE_MAX_OBS; EXPECT(clip_fuse_update_ok(f));
        f.obs_dim = CLIP_FUSE_MAX_OBS + 1; EXPECT(!clip_fuse_update_ok(f));
        printf("ok residency\n");
    }
    {   // ---- the step rule: padded rows
        EXPECT(clip_fuse_step_ok(true, 16));
        EXPECT(clip_fuse_step_ok(true, 512));
        EXPECT(!clip_fuse_step_ok(true, 528));
        EXPECT(!clip_fuse_step_ok(false, 256));
        printf("ok step_rule\n");
    }
    {   // ---- replay
        EXPECT(!clip_fuse_must_replay(true, 0));
        EXPECT(clip_fuse_must_replay(true, 1));
        EXPECT(!clip_fuse_must_replay(false, 1));            // a three-launch update never looks at the word
        const ClipFuseReplay r = clip_fuse_replay_plan(1234, 3);
        EXPECT(r.adam_t == 1234 && r.n_steps == 0 && r.pass_index == 0 && r.passes == 3);
        EXPECT(CLIP_FUSE_DEFAULT_TICKS >= 1000 && CLIP_FUSE_DEFAULT_TICKS <= 10000);   // tens of microseconds at 100 MHz
        printf("ok replay\n");
    }
    printf("checks %d\n", checks);
    return 0;
}
