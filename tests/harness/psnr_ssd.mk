# tests/harness/psnr_ssd.mk — ASan + UBSan build of psnr_ssd_check (tests/test_coded_cfg.py): the PSNR
# that DeviceWriterAsync=1 derives from the device's SSDs against psnr_pl.  A stand-alone program, all
# of it compiled from source with the sanitizers:   make -C tests/harness -f psnr_ssd.mk
CC       ?= gcc
ASAN     := _build_asan
HOSTDIR  := ../../h264-jm-commentary_amd/host
SANFLAGS := -O1 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=all
# encoder.c is included by psnr_ssd_check.c (psnr_pl is static)
HOSTSRCS := $(addprefix $(HOSTDIR)/,cfg.c yuv.c bitstream.c cabac.c deblock.c jm86.c)
HDRS     := $(HOSTDIR)/jmhost.h $(HOSTDIR)/encoder.c ../../include/jmhip.h ../../include/jmhip_coded.h

$(ASAN)/psnr_ssd_check: psnr_ssd_check.c $(HOSTSRCS) $(HDRS)
	mkdir -p $(ASAN)
	$(CC) -std=gnu99 -Wall -Wno-unused-function $(SANFLAGS) -I$(HOSTDIR) psnr_ssd_check.c $(HOSTSRCS) -o $@ -lm -lpthread
